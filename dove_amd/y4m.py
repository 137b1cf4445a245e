"""YUV4MPEG2 (.y4m) container: the codec-free stream ``ffmpeg -f yuv4mpegpipe`` reads and writes.  Host only, no dependencies.

A stream is one header line ``YUV4MPEG2 W<w> H<h> F<num>:<den> I<p> A<n>:<d> C<colourspace> X<comment>...`` and then, per frame,
``FRAME[ params]\\n`` followed by the planes Y, U, V of 8-bit samples.  Only what the GPU conversion (csrc/yuv.hip) defines is accepted:
8-bit progressive 4:2:0 / 4:2:2 / 4:4:4 / mono.  Everything else raises ``ValueError`` naming the tag and the ``ffmpeg -pix_fmt`` that
turns the clip into an accepted one.  The colour matrix is not part of Y4M; the range is (``XCOLORRANGE``, the tag ffmpeg writes)."""
from __future__ import annotations

import torch

# colourspace tag -> (chroma layout, horizontal chroma siting)
COLOURSPACES = {"C420jpeg": ("420", "centre"), "C420": ("420", "centre"), "C420mpeg2": ("420", "left"), "C420paldv": ("420", "left"),
                "C422": ("422", "left"), "C444": ("444", "left"), "Cmono": ("mono", "left")}
WRITE_TAGS = {"420": "C420jpeg", "422": "C422", "444": "C444", "mono": "Cmono"}
_MAX_HEADER = 4096


def chroma_shape(h: int, w: int, chroma: str):
    if chroma == "444":
        return h, w
    if chroma == "422":
        return h, (w + 1) // 2
    if chroma == "420":
        return (h + 1) // 2, (w + 1) // 2
    if chroma == "mono":
        return 0, 0
    raise ValueError(f"unknown chroma layout {chroma!r}: one of 444, 422, 420, mono")


def frame_bytes(h: int, w: int, chroma: str) -> int:
    ch, cw = chroma_shape(h, w, chroma)
    return h * w + 2 * ch * cw


def _fix_for(tag: str) -> str:
    body = tag[1:]
    if body.startswith("mono"):
        return "gray"
    for sub in ("444", "422", "420"):
        if body.startswith(sub) and "alpha" not in body:
            return f"yuv{sub}p"
    return "yuv444p" if body.startswith("444") else "yuv420p"


def parse_header(line: bytes) -> dict:
    """The header line (without the newline) -> dict(width, height, fps=(num, den), aspect, tag, chroma, siting_h, full_range)."""
    try:
        tokens = line.decode("ascii").split(" ")
    except UnicodeDecodeError:
        raise ValueError("not a YUV4MPEG2 stream: the header is not ASCII") from None
    if tokens[0] != "YUV4MPEG2":
        raise ValueError(f"not a YUV4MPEG2 stream: it starts with {tokens[0][:16]!r} (make one with `ffmpeg -i clip -pix_fmt yuv420p "
                         "-f yuv4mpegpipe clip.y4m`)")
    h = {"width": None, "height": None, "fps": (0, 0), "aspect": (0, 0), "tag": "C420jpeg", "full_range": False}
    for tok in tokens[1:]:
        if not tok:
            continue
        key, val = tok[0], tok[1:]
        if key == "W":
            h["width"] = int(val)
        elif key == "H":
            h["height"] = int(val)
        elif key in "FA":
            a, _, b = val.partition(":")
            h["fps" if key == "F" else "aspect"] = (int(a), int(b or 1))
        elif key == "I":
            if val not in ("p", "?"):
                raise ValueError(f"Y4M tag {tok!r}: interlaced material is not supported; deinterlace first "
                                 "(`ffmpeg -vf yadif -pix_fmt yuv420p`)")
        elif key == "C":
            if tok not in COLOURSPACES:
                what = "more than 8 bits per sample" if "p1" in val else "alpha" if "alpha" in val else "this chroma layout"
                raise ValueError(f"Y4M tag {tok!r}: {what} is not supported (accepted: {', '.join(COLOURSPACES)}); convert with "
                                 f"`ffmpeg -pix_fmt {_fix_for(tok)}`")
            h["tag"] = tok
        elif key == "X":
            if val.startswith("COLORRANGE="):
                r = val.split("=", 1)[1]
                if r not in ("FULL", "LIMITED"):
                    raise ValueError(f"Y4M tag {tok!r}: the colour range is FULL or LIMITED")
                h["full_range"] = r == "FULL"
        else:
            raise ValueError(f"Y4M tag {tok!r}: unknown header field")
    if not h["width"] or not h["height"] or h["width"] <= 0 or h["height"] <= 0:
        raise ValueError(f"Y4M header {line!r} lacks a positive W and H")
    h["chroma"], h["siting_h"] = COLOURSPACES[h["tag"]]
    return h


def _open(path_or_file, mode):
    if isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__"):
        return open(path_or_file, mode), True
    return path_or_file, False


class Y4MReader:
    """Reads frame payloads from a path or a binary file object; works on a pipe (no seek, no frame count up front)."""

    def __init__(self, src):
        self._f, self._own = _open(src, "rb")
        try:
            line = self._read_line("the stream header")
            if line is None:
                raise ValueError("not a YUV4MPEG2 stream: it is empty")
            self.header = parse_header(line)
        except Exception:
            self.close()
            raise
        self.width, self.height = self.header["width"], self.header["height"]
        self.fps, self.tag, self.chroma = self.header["fps"], self.header["tag"], self.header["chroma"]
        self.siting_h, self.full_range = self.header["siting_h"], self.header["full_range"]
        self.frame_bytes = frame_bytes(self.height, self.width, self.chroma)
        self.frames_read = 0

    def _read_line(self, what):
        """One line without its newline; None at a clean EOF (no byte read)."""
        out = bytearray()
        while True:
            b = self._f.read(1)
            if not b:
                if not out:
                    return None
                raise ValueError(f"Y4M stream ends inside {what}")
            if b == b"\n":
                return bytes(out)
            out += b
            if len(out) > _MAX_HEADER:
                raise ValueError(f"Y4M {what} is longer than {_MAX_HEADER} bytes: not a YUV4MPEG2 stream")

    def _read_into(self, view: memoryview) -> int:
        got = 0
        while got < len(view):
            n = self._f.readinto(view[got:]) if hasattr(self._f, "readinto") else None
            if n is None:                                          # file objects without readinto
                chunk = self._f.read(len(view) - got)
                n = len(chunk)
                view[got:got + n] = chunk
            if not n:
                break
            got += n
        return got

    def read(self, n: int) -> torch.Tensor:
        """Up to ``n`` frames as one uint8 tensor [k, frame_bytes] (pinned when a HIP device is present); k < n only at the end of the
        stream, k == 0 after it.  A stream that ends inside a frame raises."""
        pin = torch.cuda.is_available()
        buf = torch.empty(max(n, 0), self.frame_bytes, dtype=torch.uint8, pin_memory=pin)
        view = memoryview(buf.numpy()).cast("B") if n > 0 else None
        k = 0
        while k < n:
            line = self._read_line(f"the FRAME line of frame {self.frames_read}")
            if line is None:
                break
            if line != b"FRAME" and not line.startswith(b"FRAME "):
                raise ValueError(f"Y4M frame {self.frames_read}: expected 'FRAME', found {line[:16]!r}")
            got = self._read_into(view[k * self.frame_bytes:(k + 1) * self.frame_bytes])
            if got != self.frame_bytes:
                raise ValueError(f"Y4M frame {self.frames_read} is truncated: {got} of {self.frame_bytes} bytes")
            k += 1
            self.frames_read += 1
        return buf[:k]

    def close(self):
        if self._own:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter:
    """Writes the header once, then ``FRAME\\n`` + payload per frame, to a path or a binary file object."""

    def __init__(self, dst, width: int, height: int, fps=16, chroma: str = "444", full_range: bool = False):
        if chroma not in WRITE_TAGS:
            raise ValueError(f"unknown chroma layout {chroma!r}: one of {', '.join(WRITE_TAGS)}")
        num, den = fps if isinstance(fps, (tuple, list)) else (int(fps), 1)
        self.width, self.height, self.chroma, self.full_range = width, height, chroma, full_range
        self.frame_bytes = frame_bytes(height, width, chroma)
        self.header = (f"YUV4MPEG2 W{width} H{height} F{num}:{den} Ip A1:1 {WRITE_TAGS[chroma]} "
                       f"XCOLORRANGE={'FULL' if full_range else 'LIMITED'}\n").encode("ascii")
        self._f, self._own = _open(dst, "wb")
        self._f.write(self.header)
        self.frames_written = 0

    def write(self, payload):
        """``payload``: uint8 [k, frame_bytes] (host tensor or numpy array) or one frame's bytes."""
        if isinstance(payload, torch.Tensor):
            payload = payload.numpy()
        if isinstance(payload, (bytes, bytearray, memoryview)):
            frames = [payload]
        else:
            frames = payload.reshape(-1, self.frame_bytes)
        for fr in frames:
            if len(fr) != self.frame_bytes:
                raise ValueError(f"a {self.width}x{self.height} {self.chroma} frame is {self.frame_bytes} bytes, got {len(fr)}")
            self._f.write(b"FRAME\n")
            self._f.write(memoryview(fr))
            self.frames_written += 1

    def flush(self):
        self._f.flush()

    def close(self):
        if self._own:
            self._f.close()
        else:
            self._f.flush()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
