"""-m gpu: every attention kernel at every KV-tile count and tail class (tests/attention_cases.py: 43 lengths, 1 .. 13 tiles), two operand
families, against a float64 softmax of the same operand values:
    fwd    attn_fwd_kernel            (no score bound)                    2 heads
    pipe1  attn_pipe_kernel<1>        (bound; a launch of at most half a round of workgroups)  2 heads
    pipe2  attn_pipe_kernel<2>        (bound; just over half a round)     ceil((CUs / 2 + 1) / query blocks) heads
    mx     attn_fwd_mx_kernel         (e4m3 operands)                     2 heads
Per case: (a) closeness, (b) the kernel that ran, (c) nothing outside O written and every row of O written, (d) operand pads ignored
bit for bit, (e) pipe2 == pipe1 bit for bit on the heads they share.  Then T5's attn_bias_kernel around its tile edges and
dove_qkv_post_bf16 over the short lengths, head-group tails, text splits and both V^T packings, and dove_qkv_post_mxfp8 over the same
lengths at rounding level (tests/mx_cases.py)."""
import functools
import math

import pytest
import torch

import attention_cases as A
import emu_ops as E
from dove_amd import ops
from test_ops_gpu import close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
RTOL, AFRAC = 3e-2, 8e-3              # the attention tolerance of tests/test_ops_gpu.py against the exact softmax
PATHS = ("fwd", "pipe1", "pipe2", "mx")
GUARD = 7.0


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _guarded_out(N, heads):
    """O as rows 2 .. N + 1 of a [N + 4, heads * 64 + 4] buffer: guards 7.0, the interior NaN (an unwritten element fails `close`)."""
    ldo = heads * 64 + 4
    buf = torch.full((N + 4, ldo), GUARD, dtype=BF, device="cuda")
    buf[2:2 + N, :heads * 64] = float("nan")
    return buf, buf[2:2 + N]                                   # the second: contiguous [N, ldo]; its row length is the ldo ops.attention passes


def _check_guards(name, buf, N, heads):
    b = buf.cpu()
    mask = torch.ones(b.shape, dtype=torch.bool)
    mask[2:2 + N, :heads * 64] = False
    assert bool((b[mask].view(torch.int16) == torch.tensor(GUARD, dtype=BF).view(torch.int16)).all()), f"{name}: wrote outside O"
    return b[2:2 + N, :heads * 64].contiguous()


def _bits(t):
    return t.contiguous().view(torch.int16)


class Case:
    """One (family, N): operands for the most heads any path needs, one float64 reference, and the paths' outputs as they are computed."""

    def __init__(self, family, N):
        self.family, self.N, self.npad = family, N, A.npad(N)
        self.cus = _cus()
        self.hmax = max(2, A.pipe2_heads(N, self.cus))
        self.q, self.k, self.v = A.natural(family, N, self.hmax)
        self.Qh, self.Kh, self.Vt = A.kernel_layout(self.q, self.k, self.v)
        self.n2 = A.norm2(self.Qh, self.Kh, N)
        self.ref = A.reference(self.q, self.k, self.v)
        # (d) poisoned pads: Q and K rows [N, Npad) = 7, V^T keys >= N = 1e4 (natural order, then swapped)
        self.Qp, self.Kp = self.Qh.clone(), self.Kh.clone()
        self.Qp[:, N:] = 7.0
        self.Kp[:, N:] = 7.0
        vp = torch.full((self.hmax, 64, self.npad), 1e4, dtype=BF)
        vp[:, :, :N] = self.v
        self.Vp = E.vt_quad_swap(vp)
        self.outs = {}
        self._mx = None

    def heads(self, path):
        return self.hmax if path == "pipe2" else 2

    # ---- bf16 paths ----
    def run_bf16(self, path, poisoned=False):
        key = (path, poisoned)
        if key in self.outs:
            return self.outs[key]
        N, heads = self.N, self.heads(path)
        Q, K, V = ((self.Qp, self.Kp, self.Vp) if poisoned else (self.Qh, self.Kh, self.Vt))
        n2 = None if path == "fwd" else self.n2[:heads].clone().cuda()
        buf, out = _guarded_out(N, heads)
        ops.attention(Q[:heads].cuda(), K[:heads].cuda(), V[:heads].cuda(), N, self.npad, heads, out, norm2=n2)
        torch.cuda.synchronize()
        want = "attn_fwd_kernel" if path == "fwd" else "attn_pipe_kernel"
        assert ops.attention_head_paths(n2, heads) == [want] * heads                                   # (b)
        got = _check_guards(f"{path}{'_poisoned' if poisoned else ''}", buf, N, heads)                   # (c)
        self.outs[key] = got
        return got

    # ---- MXFP8 path: operands as tests/test_ops_gpu.py test_attention_mx_spike_and_flat_tail builds them ----
    def mx_operands(self):
        if self._mx is None:
            N, npad, heads = self.N, self.npad, 2
            u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
            Q8, K8 = u8(heads, npad, 64), u8(heads, npad, 64)
            Q8[:, :N] = (self.q[:heads].float() * 8).to(torch.float8_e4m3fn).view(torch.uint8)
            K8[:, :N] = self.k[:heads].float().to(torch.float8_e4m3fn).view(torch.uint8)
            vp = torch.zeros(heads * 64, npad)
            vp[:, :N] = self.v[:heads].float().reshape(heads * 64, N)
            vq, ve = E.mx_quant_ref(vp)
            vq8 = vq.view(torch.uint8).reshape(heads, 64, npad)
            V8 = E.v8_store_order(vq8).contiguous()
            Vs = ve.reshape(heads, 64, npad // 64, 2).permute(0, 2, 1, 3).contiguous()
            # poisoned pads: e4m3 7.0 in the Q / K pad rows; V keys >= N = 448 (the largest e4m3), blocks wholly in the pad scaled by 2^7
            seven = int(torch.tensor(7.0).to(torch.float8_e4m3fn).view(torch.uint8))
            Qp, Kp, vqp, vep = Q8.clone(), K8.clone(), vq8.clone(), ve.clone()
            Qp[:, N:] = seven
            Kp[:, N:] = seven
            vqp[:, :, N:] = 0x7E
            vep[:, (N + 31) // 32:] = 127 + 7
            Vp = E.v8_store_order(vqp).contiguous()
            Vsp = vep.reshape(heads, 64, npad // 64, 2).permute(0, 2, 1, 3).contiguous()
            deq = E.mx_dequant(vq, ve).reshape(heads, 64, npad)[:, :, :N]
            qd = Q8.view(torch.float8_e4m3fn).float()[:, :N] * 0.125
            kd = K8.view(torch.float8_e4m3fn).float()[:, :N]
            self._mx = dict(clean=(Q8, K8, V8, Vs), poisoned=(Qp, Kp, Vp, Vsp), exact=A.reference(qd, kd, deq))
        return self._mx

    def run_mx(self, poisoned=False):
        key = ("mx", poisoned)
        if key in self.outs:
            return self.outs[key]
        N, heads = self.N, 2
        opnd = self.mx_operands()["poisoned" if poisoned else "clean"]
        buf, out = _guarded_out(N, heads)
        ops.attention_mx(*(t.cuda() for t in opnd), N, self.npad, heads, out)
        torch.cuda.synchronize()
        got = _check_guards(f"mx{'_poisoned' if poisoned else ''}", buf, N, heads)
        self.outs[key] = got
        return got


@functools.lru_cache(maxsize=1)
def _case(family, N):
    return Case(family, N)


def _rel_rms(x, exact):
    return float((x.double() - exact).pow(2).mean().sqrt() / exact.pow(2).mean().sqrt())


CASES = [(N, f, p) for N in A.LENGTHS for f in A.FAMILIES for p in PATHS]      # the path varies fastest: one operand set per (N, family)


@pytest.mark.parametrize("N,family,path", CASES, ids=[f"{N}-{f}-{p}" for N, f, p in CASES])
def test_attention_length(N, family, path):
    c = _case(family, N)
    name = f"attention_{path}_{family}_{N}"
    if path == "mx":
        got = c.run_mx()                                                                              # (c) inside
        mx = c.mx_operands()
        emu = E.attention_mx(*mx["clean"], N, c.npad, 2, torch.zeros(N, 128, dtype=BF))
        rk, re = _rel_rms(got, mx["exact"]), _rel_rms(emu, mx["exact"])
        print(f"[mx] N={N} {family}: rel RMS vs exact softmax of the dequantised operands: kernel {rk:.4e}, restatement {re:.4e}")
        close(name, got, emu, rtol=4e-2, afrac=2e-2, max_bad=max(2, got.numel() // 200000))          # (a)
        assert rk <= 1.25 * re + 1e-3, (rk, re)
        assert torch.equal(_bits(c.run_mx(poisoned=True)), _bits(got)), f"{name}: the operand pads changed the result"   # (d)
        return
    heads = c.heads(path)
    items = A.qblocks(N) * heads
    if path == "pipe1":
        assert A.pipe_form(N, heads, c.cus) == (0, items)
    if path == "pipe2":
        assert A.pipe_form(N, heads, c.cus) == (items, 0)                                             # every item on attn_pipe_kernel<2>
    got = c.run_bf16(path)                                                                            # (b), (c) inside
    ratio = A.tolerance_ratio(got, c.ref[:, :heads * 64], RTOL, AFRAC)
    print(f"[{path}] N={N} {family}: worst error / tolerance {float(torch.nan_to_num(ratio, nan=math.inf).max()):.3f}")
    close(name, got, c.ref[:, :heads * 64], rtol=RTOL, afrac=AFRAC, max_bad=0)                         # (a)
    assert torch.equal(_bits(c.run_bf16(path, poisoned=True)), _bits(got)), f"{name}: the operand pads changed the result"   # (d)
    if path == "pipe2":
        assert torch.equal(_bits(got[:, :128]), _bits(c.run_bf16("pipe1"))), f"{name}: <2> and <1> differ on the same rows"  # (e)


@pytest.mark.parametrize("N", [1, 5, 63, 64, 65, 127, 128, 129, 1024])
def test_attention_bias_lengths(N):
    H = 2
    g = torch.Generator().manual_seed(40 + N)
    qkv = (torch.randn(N, 3 * H * 64, generator=g) * 0.5).to(BF)
    bias = torch.randn(H, N, N, generator=g) * 2
    # P is rounded to bf16 on both sides: 2 ulp (tests/test_t5_gpu.py test_t5_operators)
    close(f"attention_bias_{N}", ops.attention_bias(qkv.cuda(), bias.cuda(), H), E.attention_bias(qkv, bias, H), rtol=3e-2, afrac=8e-3)


def _guarded(shape, dtype, pad=64):
    """A zero tensor of `shape` inside a flat buffer with `pad` guard elements (7) on either side."""
    n = math.prod(shape)
    flat = torch.full((n + 2 * pad,), GUARD, dtype=dtype, device="cuda")
    flat[pad:pad + n] = 0
    return flat, flat[pad:pad + n].view(*shape)


def _guards_intact(flat, n, pad=64):
    f = flat.cpu()
    return bool((f[:pad] == GUARD).all()) and bool((f[pad + n:] == GUARD).all())


QKV_LENGTHS = [N for N in A.LENGTHS if A.ntiles(N) <= 5]
QKV_CASES = [(N, heads, tl, packing, v_order)
             for N in QKV_LENGTHS for heads in (1, 9) for tl in sorted({0, min(226, N), N})
             for packing, v_order in (("pad128", 1), ("pad128", 0), ("local", 0))]


@pytest.mark.parametrize("N,heads,text_len,packing,v_order", QKV_CASES, ids=["-".join(map(str, c)) for c in QKV_CASES])
def test_qkv_post_lengths(N, heads, text_len, packing, v_order):
    """dove_qkv_post_bf16 against its restatement.  heads = 9: the second group of eight heads holds one live head.  "local": the
    rank-local packing Npad == N of dove_amd.dist - with N % 8 != 0 the V^T rows are not 16-byte aligned and go out as two-byte stores."""
    D = heads * 64
    npad = A.npad(N) if packing == "pad128" else N
    g = torch.Generator().manual_seed(7 * N + heads)
    qkv = torch.randn(N, 3 * D, generator=g).to(BF)
    gq, bq, gk, bk = (1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g),
                      1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g))
    ang = torch.rand(max(N - text_len, 1), 32, generator=g) * 6.28
    cos, sin = ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous()
    if heads == 9:                                              # a table whose pair entries differ: cr[2i + 1] for cr[2i] is then visible
        ang = torch.rand(max(N - text_len, 1), 64, generator=g) * 6.28
        cos, sin = ang.cos().contiguous(), (ang + 0.3 * torch.randn(ang.shape, generator=g)).sin().contiguous()
    qscale = 0.125 * math.log2(math.e)
    z = lambda *s: torch.zeros(*s, dtype=BF)   # noqa: E731
    Qr, Kr, Vr = z(heads, npad, 64), z(heads, npad, 64), z(heads, 64, npad)
    E.qkv_post(qkv, N, npad, heads, text_len, gq, bq, gk, bk, cos, sin, qscale, 1e-6, Qr, Kr, Vr, v_order=v_order)
    (fq, Qg), (fk, Kg), (fv, Vg) = _guarded((heads, npad, 64), BF), _guarded((heads, npad, 64), BF), _guarded((heads, 64, npad), BF)
    fn, n2 = _guarded((heads, 2), torch.float32)
    n2.fill_(-1.0)                                              # stale contents: the call clears the array itself
    ops.qkv_post(qkv.cuda(), N, npad, heads, text_len, gq.cuda(), bq.cuda(), gk.cuda(), bk.cuda(), cos.cuda(), sin.cuda(),
                 qscale, 1e-6, Qg, Kg, Vg, v_order=v_order, norm2=n2)
    torch.cuda.synchronize()
    close("qkv_post.Q", Qg, Qr)
    close("qkv_post.K", Kg, Kr)
    assert torch.equal(Vg.cpu(), Vr), "V^T is a copy: must be bit-exact, pad columns zero"
    assert not bool(Qg[:, N:].any()) and not bool(Kg[:, N:].any()), "pre-zeroed pad rows were written"
    want = torch.stack([(Qg[:, :N].float() ** 2).sum(-1).amax(-1), (Kg[:, :N].float() ** 2).sum(-1).amax(-1)], dim=1)
    assert torch.allclose(n2, want, rtol=1e-5, atol=0), (n2, want)
    for nm, flat, n in (("Qh", fq, Qg.numel()), ("Kh", fk, Kg.numel()), ("Vt", fv, Vg.numel()), ("norm2", fn, n2.numel())):
        assert _guards_intact(flat, n), f"{nm}: wrote outside the buffer"


def _guarded_u8(shape, pad=256):
    """A uint8 tensor of `shape` prefilled with 0x55 inside a flat buffer with `pad` guard bytes (0xA7) on either side."""
    n = math.prod(shape)
    flat = torch.full((n + 2 * pad,), 0xA7, dtype=torch.uint8, device="cuda")
    flat[pad:pad + n] = 0x55
    return flat, flat[pad:pad + n].view(*shape)


QKV_MX_CASES = [(N, heads, tl, rope) for N in QKV_LENGTHS for heads in (1, 9) for tl in sorted({0, min(226, N), N}) for rope in (True, False)]


@pytest.mark.parametrize("N,heads,text_len,rope", QKV_MX_CASES, ids=["-".join(map(str, c)) for c in QKV_MX_CASES])
def test_qkv_post_mx_lengths(N, heads, text_len, rope):
    """dove_qkv_post_mxfp8 over the same lengths (Npad = the next multiple of 128, all the entry point takes): V8t / Vs bit-exact against the
    exact MX rule of tests/mx_cases.py in the stored quad order, pad keys and whole pad tiles zero bytes with scale byte 0; Q8 / K8 within
    0.5 ulp_e4m3 + k 2^-24 mag of a float64 LayerNorm + RoPE + scale, pad rows zero; cos / sin tables whose pair entries differ, or none.
    All four outputs are guarded views prefilled with 0x55: the guards stay and every byte of [heads][Npad] is rewritten."""
    import mx_cases as MC
    npad = A.npad(N)
    qkv, aff, cos, sin = MC.qkv_operands(N, heads, text_len, rope)
    qscale = 0.125 * math.log2(math.e)
    Qr, mQ, Kr, mK = MC.qkv_ref64(qkv, N, heads, text_len, aff, cos, sin, qscale, 1e-6)
    V8r, Vsr = MC.v_exact(qkv, N, npad, heads)
    (fq, Q8), (fk, K8) = _guarded_u8((heads, npad, 64)), _guarded_u8((heads, npad, 64))
    (fv, V8), (fs, Vs) = _guarded_u8((heads, 64, npad)), _guarded_u8((heads, npad // 64, 64, 2))
    dev = lambda t: None if t is None else t.cuda()   # noqa: E731
    ops.qkv_post_mx(qkv.cuda(), N, npad, heads, text_len, *(t.cuda() for t in aff), dev(cos), dev(sin), qscale, 1e-6, Q8, K8, V8, Vs)
    torch.cuda.synchronize()
    for nm, flat, t in (("Q8", fq, Q8), ("K8", fk, K8), ("V8t", fv, V8), ("Vs", fs, Vs)):
        f = flat.cpu()
        assert bool((f[:256] == 0xA7).all()) and bool((f[256 + t.numel():] == 0xA7).all()), f"{nm}: wrote outside the buffer"
    assert torch.equal(V8.cpu(), V8r), "V8t differs from the exact rule"
    assert torch.equal(Vs.cpu(), Vsr), "Vs differs from the exact rule"
    assert not bool(V8[:, :, N:].any()) and not bool(Vs.cpu().reshape(heads, npad // 64, 64, 2).permute(0, 2, 1, 3).reshape(heads, 64, npad // 32)
                                                     [:, :, (N + 31) // 32:].any()), "pad keys / pad blocks are not zero"
    for nm, got8, ref, mag in (("Q8", Q8, Qr, mQ), ("K8", K8, Kr, mK)):
        g = got8.cpu()
        assert not bool(g[:, N:].any()), f"{nm}: pad rows are not zero"
        got = g[:, :N].contiguous().view(torch.float8_e4m3fn).float().double()
        assert bool(torch.isfinite(got).all()), f"{nm}: a byte was never written or is NaN"
        err, tol = (got - ref).abs(), MC.qkv_budget(ref, mag)
        bad = ~(err <= tol)
        assert not bool(bad.any()), (f"{nm}: {int(bad.sum())}/{bad.numel()} over the budget, worst {float((err / tol).max()):.3g}x; needs k "
                                     f"{float(((err - 0.5 * MC.ulp_e4m3(ref)).clamp_min(0) / (MC.EPS24 * mag)).max()):.1f}")
