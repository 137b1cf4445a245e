"""Cases for the attention kernels' tile loops (pure torch / Python, no GPU): the sequence lengths that reach every loop class, the
classes themselves, the launch rule of the pipelined kernel, two seeded operand families in the kernels' layout and a float64 reference.

The kernels walk 64-key tiles, ntiles = ceil(N / 64):
  attn_pipe_kernel (attention_pipe.hip): main trips of four unmasked steps while j + 4 <= last_full, then one or two masked tail trips;
  attn_fwd_kernel / attn_fwd_mx_kernel (attention.hip, attention_mx.hip): four tiles per trip in two barrier phases, `break` between them.
The functions below RESTATE that arithmetic - a change of the loops has to be mirrored here, and tests/test_attention_cases_cpu.py checks
that LENGTHS still reaches every class."""
import math

import torch

import emu_ops as E

BF = torch.bfloat16
TILE = 64
MAX_TILES = 13


def _lengths():
    out = []
    for t in range(1, MAX_TILES + 1):
        base = TILE * (t - 1)
        out += [base + 1, base + 33, base + TILE]               # one key / one key past a 32-key half / a full last tile
        if t in (2, 6):
            out += [base + 32, base + 63]                       # exactly one half / one key short
    return sorted(out)


LENGTHS = _lengths()
FAMILIES = ("dense", "selector")


def ntiles(N):
    return (N + TILE - 1) // TILE


def npad(N):
    return (N + 127) // 128 * 128


def pipe_class(N):
    """attn_pipe_kernel: (ntiles mod 4, ragged last tile, main trips 0 / 1 / 2 = two or more, tail trips)."""
    nt = ntiles(N)
    ragged = N % TILE != 0
    last_full = nt - 1 - (1 if ragged else 0)                   # highest tile index that needs no mask (-1: none)
    j = main = 0
    while j + 4 <= last_full:
        j += 4
        main += 1
    tail = 0
    while j < nt:
        j += 4
        tail += 1
    assert tail in (1, 2)
    return (nt % 4, ragged, min(main, 2), tail)


def fwd_class(N):
    """attn_fwd_kernel and attn_fwd_mx_kernel: (how the loop ends, tiles in the last barrier phase, mask taken, whole trips before the last:
    0 / 1 / 2 = two or more).  "break": the last trip leaves between its two phases; "end": it runs both and the loop condition ends it."""
    nt = ntiles(N)
    it = whole = 0
    while True:
        assert it < nt
        if it + 2 >= nt:                                        # first phase computes tiles it, it + 1 (if it exists), then breaks
            exit_, last = "break", nt - it
            break
        if it + 4 >= nt:                                        # second phase computes it + 2, it + 3 (if it exists); the loop ends
            exit_, last = "end", nt - it - 2
            break
        it += 4
        whole += 1
    assert last in (1, 2)
    return (exit_, last, N % TILE != 0, min(whole, 2))


def pipe_form(N, heads, cus):
    """dove_attention_pipe_launch: (items on attn_pipe_kernel<2>, items on attn_pipe_kernel<1>); an item = (head, 256-query block)."""
    items = (npad(N) + 255) // 256 * heads
    rem = items % cus
    if 2 * rem > cus:
        rem = 0
    return items - rem, rem


def qblocks(N):
    return (npad(N) + 255) // 256


def pipe2_heads(N, cus):
    """The fewest heads whose items make a last round of more than half the CUs - which stays on attn_pipe_kernel<2>."""
    return -(-(cus // 2 + 1) // qblocks(N))


def _seed(family, N):
    return 1000 * N + FAMILIES.index(family)


def natural(family, N, heads):
    """q, k [heads, N, 64] and v [heads, 64, N] (natural key order) in bf16.
    dense:    q ~ 0.5 N(0,1), k ~ N(0,1), v ~ N(0,1): scores ~ N(0, 4^2) in base 2.
    selector: u_j random unit vectors, k_j = sqrt(24) u_j, q_i = sqrt(24) u_(N-1-i): query i scores 24 on key N-1-i and ~N(0, 3^2) elsewhere,
              so every key is the near-exclusive target (p >= 0.999) of exactly one query and a dropped, duplicated or misplaced key or V^T
              column shows in that query's row at every N.  Bound ~24, row sums ~2^24: inside the no-shift kernel's window."""
    g = torch.Generator().manual_seed(_seed(family, N))
    if family == "dense":
        q = torch.randn(heads, N, 64, generator=g) * 0.5
        k = torch.randn(heads, N, 64, generator=g)
    elif family == "selector":
        u = torch.randn(heads, N, 64, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        k = math.sqrt(24.0) * u
        q = math.sqrt(24.0) * u.flip(1)
    else:
        raise ValueError(family)
    v = torch.randn(heads, 64, N, generator=g)
    return q.to(BF), k.to(BF), v.to(BF)


def kernel_layout(q, k, v):
    """-> Qh, Kh [heads, Npad, 64], Vt [heads, 64, Npad] quad-swapped; pads zero (dove_attention_fwd_bf16's operand contract)."""
    heads, N = q.shape[0], q.shape[1]
    P = npad(N)
    Qh = torch.zeros(heads, P, 64, dtype=BF)
    Kh = torch.zeros(heads, P, 64, dtype=BF)
    Vt = torch.zeros(heads, 64, P, dtype=BF)
    Qh[:, :N], Kh[:, :N], Vt[:, :, :N] = q, k, v
    E.vt_quad_swap(Vt)
    return Qh, Kh, Vt


def norm2(Qh, Kh, N):
    """The score bound as dove_qkv_post_bf16 leaves it: max squared norms of the stored rows [heads, 2]."""
    return torch.stack([(Qh[:, :N].float() ** 2).sum(-1).amax(-1), (Kh[:, :N].float() ** 2).sum(-1).amax(-1)], dim=1).contiguous()


def reference(q, k, v, chunk=8):
    """float64 softmax(q k^T ln 2) v of the operand VALUES (q carries scale * log2 e): q, k [heads, Nq|Nk, 64], v [heads, 64, Nk] in natural
    key order -> [Nq, heads * 64] float64.  Independent of emu_ops.attention."""
    heads, nq = q.shape[0], q.shape[1]
    out = torch.empty(nq, heads * 64, dtype=torch.float64)
    for h0 in range(0, heads, chunk):
        qq, kk, vv = (t[h0:h0 + chunk].to(torch.float64) for t in (q, k, v))
        s = torch.matmul(qq, kk.transpose(1, 2)) * math.log(2.0)
        p = torch.softmax(s, dim=-1)
        o = torch.matmul(p, vv.transpose(1, 2))                 # [h, Nq, 64]
        out[:, h0 * 64:(h0 + o.shape[0]) * 64] = o.permute(1, 0, 2).reshape(nq, -1)
    return out


def flash_emulation(q, k, v):
    """What a correct flash kernel may do to the exact result: 64-key tiles, running maximum, P rounded to bf16 before PV, fp32 sums,
    one bf16 rounding of the output.  -> [N, heads * 64] bf16."""
    heads, N = q.shape[0], q.shape[1]
    qf, kf, vf = q.float(), k.float(), v.float()
    m = torch.full((heads, N), -math.inf)
    l = torch.zeros(heads, N)
    o = torch.zeros(heads, N, 64)
    for t0 in range(0, k.shape[1], TILE):
        s = torch.matmul(qf, kf[:, t0:t0 + TILE].transpose(1, 2))
        mn = torch.maximum(m, s.amax(-1))
        alpha = torch.exp2(m - mn)
        p = torch.exp2(s - mn[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + torch.matmul(p.to(BF).float(), vf[:, :, t0:t0 + TILE].transpose(1, 2))
        m = mn
    return (o / l[..., None]).permute(1, 0, 2).reshape(N, heads * 64).to(BF)


def tolerance_ratio(got, ref, rtol, afrac):
    """|got - ref| / (rtol |ref| + afrac max |ref| + 1e-6) per element: the quantity test_ops_gpu.close() compares with 1."""
    got, ref = got.double(), ref.double()
    return (got - ref).abs() / (rtol * ref.abs() + afrac * ref.abs().max() + 1e-6)
