"""A RIFF AVI 1.0 writer for Motion-JPEG: host-side bookkeeping around the files ``dove_amd.jpeg`` encodes.

    RIFF 'AVI ' > LIST 'hdrl' (avih, LIST 'strl' (strh: vids / MJPG, scale / rate = 1 / fps; strf: BITMAPINFOHEADER, MJPG, 24 bits))
                > LIST 'movi' of '00dc' chunks, each one complete JPEG file, padded to even length
                > idx1 (AVIIF_KEYFRAME, offsets relative to the 'movi' fourcc)

Frames are appended one at a time, so a clip is never held as bytes twice; the sizes and the frame count are patched on ``close``, which
needs a seekable file.  AVI 1.0 ends at 4 GiB; OpenDML is not written, and ``write`` raises before a file would pass that limit."""
from __future__ import annotations

import struct

RIFF_LIMIT = (1 << 32) - 1          # a RIFF size field is 32 bits and counts the bytes after it
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
_HDRL_BYTES = 4 + (8 + 56) + (12 + (8 + 56) + (8 + 40))      # 'hdrl' + avih + LIST strl (strh, strf)
_MOVI_LIST_AT = 12 + 8 + _HDRL_BYTES                          # file offset of the 'LIST' that holds 'movi'


class AviError(ValueError):
    pass


class MjpegAviWriter:
    """``MjpegAviWriter(path, width, height, fps)``; ``write(jpeg_bytes)`` per frame; ``close()`` (or a ``with`` block)."""

    def __init__(self, path, width: int, height: int, fps):
        if path == "-" or path is None:
            raise AviError("an AVI file has its sizes patched when it is closed: it needs a seekable file, not '-'")
        fps = int(fps)
        if fps <= 0 or width <= 0 or height <= 0:
            raise AviError(f"avi: bad width {width}, height {height} or fps {fps}")
        self.width, self.height, self.fps = int(width), int(height), fps
        self._own = isinstance(path, (str, bytes)) or hasattr(path, "__fspath__")
        self._f = open(path, "wb") if self._own else path
        if not self._own and not (hasattr(self._f, "seekable") and self._f.seekable()):
            raise AviError("an AVI file has its sizes patched when it is closed: it needs a seekable file")
        self._index = []                                      # (offset relative to the 'movi' fourcc, size) per frame
        self._max = 0
        self._movi = 4                                        # bytes of the movi list's data so far: its fourcc
        self._closed = False
        self._f.write(self._headers(0, 0, 0))

    def _headers(self, riff_size: int, movi_size: int, frames: int) -> bytes:
        w, h, fps = self.width, self.height, self.fps
        avih = struct.pack("<14I", 1000000 // fps, self._max * fps, 0, AVIF_HASINDEX, frames, 0, 1, self._max, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, 1, fps, 0, frames, self._max, 0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        assert len(hdrl) == _HDRL_BYTES
        return (b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
                + b"LIST" + struct.pack("<I", movi_size) + b"movi")

    def _final_size(self, movi: int, frames: int) -> int:
        """The RIFF size field if the file were closed with ``movi`` bytes of movi data and ``frames`` frames."""
        return 4 + 8 + _HDRL_BYTES + 8 + movi + 8 + 16 * frames

    def write(self, jpeg: bytes) -> None:
        if self._closed:
            raise AviError("avi: the file is closed")
        n = len(jpeg)
        padded = n + (n & 1)
        if self._final_size(self._movi + 8 + padded, len(self._index) + 1) > RIFF_LIMIT:
            raise AviError(f"avi: frame {len(self._index)} would take the file past the 4 GiB limit of RIFF AVI 1.0 (OpenDML is not written); "
                           "split the clip")
        self._f.write(b"00dc" + struct.pack("<I", n))
        self._f.write(jpeg)
        if n & 1:
            self._f.write(b"\0")
        self._index.append((self._movi, n))
        self._movi += 8 + padded
        self._max = max(self._max, n)

    @property
    def frames(self) -> int:
        return len(self._index)

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        idx = b"".join(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, n) for off, n in self._index)
        self._f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        self._f.seek(0)
        self._f.write(self._headers(self._final_size(self._movi, len(self._index)), self._movi, len(self._index)))
        self._f.seek(0, 2)
        if self._own:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
