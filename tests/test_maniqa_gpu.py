"""MANIQA on the GPU (csrc/maniqa.hip, dove_amd/maniqa.py): the batched GEMM, the row softmax, the window attention, the stages at production
width and the tiny network inside 20 x the deviation of the restatement's (tests/maniqa_ref.py) own fp32 run from its fp64 run on the same
inputs (test_fastvqa_gpu.gate_check), the GEMM's exact cases and its fmaf chain bit for bit, the gathers bit for bit, and the tool."""
import gc
import json

import numpy as np
import pytest
import torch

import maniqa_ref as R
import test_maniqa_cpu as T
from dove_amd import fastvqa, ops, prepost
from dove_amd import maniqa as Q
from test_fastvqa_gpu import gate_check

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32 = torch.float64, torch.float32
_CACHE = {}


def _drop_device_tables():
    for geo in list(fastvqa._GEOMETRY.values()) + list(Q._ORIGINS.values()):
        geo["device"].clear()


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory():
    """test_dover_gpu's fixture for this module: the weights and the geometry tables stay on the device while the module runs; drop them
    when it is done and check that device memory returns to its level before the module.  The module allocates from a memory pool of its
    own, released with it, so that the caching allocator is left exactly as it was found, its cached free blocks included
    (test_stream_gpu.test_bounded_memory compares peaks of ``memory_allocated``)."""
    live, reserved = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
        _CACHE.clear()
        _drop_device_tables()
        gc.collect()
        torch.cuda.synchronize()
    del pool
    print(f"device memory after the module: allocated {torch.cuda.memory_allocated()} (before: {live}), reserved "
          f"{torch.cuda.memory_reserved()} (before: {reserved})")
    assert torch.cuda.memory_allocated() <= live, "this module left tensors on the device"
    assert torch.cuda.memory_reserved() <= reserved, "this module left segments in the allocator"


def part(*prefixes, cfg=None):
    """(state dict, weights) of the named parts of the production (or a given) network's random state."""
    cfg = Q.CFG if cfg is None else cfg
    key = (prefixes, tuple(sorted((k, str(v)) for k, v in cfg.items())))
    if key not in _CACHE:
        sd = Q.random_state(cfg, 5, only=prefixes)
        _CACHE[key] = (sd, Q.ManiqaWeights.from_state_dict(sd, cfg, partial=True).to(DEV))
    return _CACHE[key]


def tiny():
    if "tiny" not in _CACHE:
        _CACHE["tiny"] = (T.state(), Q.ManiqaWeights.from_state_dict(T.state(), T.TINY))
    return _CACHE["tiny"]


def rnd(seed, *shape, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- 1. the batched GEMM ----------------------------------------------------------------------------------------------------------------
def _bmm_ref(a, b, bt, bias, bias_rows, res, alpha, tr, dtype):
    a, b = a.to(dtype), b.to(dtype)
    y = a @ (b.transpose(-2, -1) if bt else b)
    if alpha != 1.0:
        y = y * alpha
    if bias is not None:
        y = y + (bias.to(dtype)[:, None] if bias_rows else bias.to(dtype))
    y = y.transpose(-2, -1) if tr else y
    return y + res.to(dtype) if res is not None else y


# (batch, M, N, K, B transposed, shared B): a single output; K % 32 == 16 with row and column tails; tails on every side with K = 32 + 20;
# a weight shared by the batch (batch stride 0)
BMM_CASES = [(1, 1, 4, 4, False, False), (1, 1, 4, 4, True, False), (2, 33, 20, 784, False, False), (3, 130, 132, 52, True, False),
             (2, 70, 24, 36, False, True), (2, 70, 24, 36, True, True)]


@pytest.mark.parametrize("case", BMM_CASES, ids=str)
def test_bmm_against_fp64(case):
    B, M, N, K, bt, shared = case
    a = rnd(7000 + M + K, B, M, K)
    b = rnd(7001 + N + K, *(() if shared else (B,)), *((N, K) if bt else (K, N)))
    ad, bd = a.to(DEV), b.to(DEV)
    for bias_rows, with_res, alpha, tr in ((False, False, 1.0, False), (False, True, 0.25, False), (True, False, 1.0, True), (False, True, 1.5, True),
                                           (True, True, 1.0, False)):
        bias = rnd(7002, M if bias_rows else N)
        res = rnd(7003, B, N, M) if tr else rnd(7003, B, M, N)
        for use_bias in (False, True):
            args = (bt, bias if use_bias else None, bias_rows, res if with_res else None, alpha, tr)
            got = ops.bmm_f32(ad, bd, b_transposed=bt, bias=bias.to(DEV) if use_bias else None, bias_rows=bias_rows,
                              residual=res.to(DEV) if with_res else None, alpha=alpha, store_transposed=tr)
            assert tuple(got.shape) == ((B, N, M) if tr else (B, M, N))
            gate_check(f"bmm {case} bias {use_bias} rows {bias_rows} residual {with_res} alpha {alpha} transposed store {tr}", got,
                       _bmm_ref(a, b, *args, F64), _bmm_ref(a, b, *args, F32))


@pytest.mark.parametrize("case", [(3072, 3072, 784, True), (3072, 784, 3072, False)], ids=str)
def test_bmm_production_shapes(case):
    M, N, K, bt = case
    a, b = rnd(7100 + K, M, K), rnd(7101 + N, *((N, K) if bt else (K, N)))
    got = ops.bmm_f32(a.to(DEV), b.to(DEV), b_transposed=bt, alpha=float(K) ** -0.5)
    gate_check(f"bmm {case}", got, _bmm_ref(a, b, bt, None, False, None, float(K) ** -0.5, False, F64),
               _bmm_ref(a, b, bt, None, False, None, float(K) ** -0.5, False, F32))


def test_bmm_exact_cases():
    K = 52                                                                                     # one whole K step and a short one
    b = rnd(7200, K, 36)                                                                       # asymmetric: a swapped store would show
    eye = torch.eye(K)
    bd = b.to(DEV)
    assert torch.equal(ops.bmm_f32(eye.to(DEV), bd).cpu(), b)                                  # I B = B, bit for bit
    assert torch.equal(ops.bmm_f32(eye.to(DEV), bd, store_transposed=True).cpu(), b.t())
    assert torch.equal(ops.bmm_f32(eye.to(DEV), b.t().contiguous().to(DEV), b_transposed=True).cpu(), b)
    a = rnd(7201, 133, K)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(7202))
    onehot = torch.zeros(K, K)
    onehot[perm, torch.arange(K)] = 1.0                                                        # column j picks k = perm[j]
    assert torch.equal(ops.bmm_f32(a.to(DEV), onehot.to(DEV)).cpu(), a[:, perm])
    assert torch.equal(ops.bmm_f32(a.to(DEV), onehot.t().contiguous().to(DEV), b_transposed=True).cpu(), a[:, perm])
    # the chain itself: operands of 12 significant bits, whose fmaf chain tests/maniqa_ref.py emulates exactly
    for bt in (False, True):
        x, w = R.short_mantissa(rnd(7203, 37, K)), R.short_mantissa(rnd(7204, K, 20))
        got = ops.bmm_f32(x.to(DEV), (w.t().contiguous() if bt else w).to(DEV), b_transposed=bt).cpu()
        diff = int((got != R.fmaf_chain(x, w)).sum())
        print(f"bmm 37 x 20 x {K} (B transposed: {bt}): {diff} of {got.numel()} outputs differ from the emulated k-ascending fmaf chain")
        assert diff == 0
    # batch independence, shared operands and a repeat call
    A, Bm = rnd(7205, 3, 70, 36).to(DEV), rnd(7206, 3, 36, 24).to(DEV)
    got = ops.bmm_f32(A, Bm)
    assert torch.equal(ops.bmm_f32(A, Bm), got) and torch.equal(ops.bmm_f32(A[1:], Bm[1:]), got[1:])
    assert torch.equal(ops.bmm_f32(A[2], Bm[2]), got[2])
    assert torch.equal(ops.bmm_f32(A, Bm[1]), ops.bmm_f32(A, Bm[1:2].expand(3, -1, -1)))       # a 2-D operand is a batch stride of 0
    assert torch.equal(ops.bmm_f32(A, Bm[1])[0], ops.bmm_f32(A[0], Bm[1]))
    wide = rnd(7207, 3, 70, 80).to(DEV)                                                        # column slices of a wider buffer
    assert torch.equal(ops.bmm_f32(wide[..., 4:40], Bm), ops.bmm_f32(wide[..., 4:40].contiguous(), Bm))
    # the residual may be out; out may not be an operand
    res = rnd(7208, 3, 70, 24).to(DEV)
    want = ops.bmm_f32(A, Bm, residual=res)
    buf = res.clone()
    assert ops.bmm_f32(A, Bm, residual=buf, out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, want)
    sq = rnd(7209, 2, 24, 24).to(DEV)
    with pytest.raises(ValueError, match="must not alias a or b"):
        ops.bmm_f32(sq, sq.clone(), out=sq)
    flat = torch.zeros(2 * 24 * 24 + 24, device=DEV)                                           # b and out overlap in part
    with pytest.raises(ValueError, match="must not alias a or b"):
        ops.bmm_f32(sq, flat[24:].view(2, 24, 24), out=flat[:2 * 24 * 24].view(2, 24, 24))
    with pytest.raises(ValueError, match="residual must not alias out"):
        flat = torch.zeros(2 * 24 * 24 + 8, device=DEV)
        ops.bmm_f32(sq, sq.clone(), residual=flat[8:].view(2, 24, 24), out=flat[:2 * 24 * 24].view(2, 24, 24))
    with pytest.raises(ValueError, match="multiples of 4"):
        ops.bmm_f32(rnd(1, 5, 6).to(DEV), rnd(2, 6, 8).to(DEV))


# ---- 2. the row softmax -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (7, 130), (5, 3072), (3, 768)], ids=str)
def test_softmax_rows(shape):
    R_, Cc = shape
    x = rnd(7300 + Cc, R_, Cc, scale=3.0)
    if R_ >= 3:
        x[0, Cc // 3] = 80.0                                                                   # a row whose maximum is + 80 ...
        x[1] = -80.0                                                                           # ... and one whose entries are all - 80
    xd = x.to(DEV)
    got = ops.softmax_rows_f32(xd)
    assert bool(torch.isfinite(got).all())
    gate_check(f"softmax {shape}", got, x.double().softmax(-1), x.softmax(-1))
    gate_check(f"softmax {shape}: row sums", got.double().sum(-1), torch.ones(R_, dtype=F64), x.softmax(-1).double().sum(-1))
    if R_ >= 3:
        assert torch.equal(got[1].cpu(), torch.full((Cc,), 1.0 / Cc)) and float(got[0, Cc // 3]) > 0.99
    wide = torch.zeros(R_, Cc + 5, device=DEV)
    wide[:, :Cc] = xd
    assert torch.equal(ops.softmax_rows_f32(wide[:, :Cc]), got) and torch.equal(ops.softmax_rows_f32(xd), got)
    assert ops.softmax_rows_f32(xd, out=xd).data_ptr() == xd.data_ptr() and torch.equal(xd, got)


# ---- 3. the window attention ------------------------------------------------------------------------------------------------------------
def _window_ref(qkv, heads, table, index, region, dtype):
    Wn, N, D3 = qkv.shape
    d = D3 // (3 * heads)
    q, k, v = (t.reshape(Wn, N, heads, d).transpose(1, 2) for t in qkv.to(dtype).split(D3 // 3, dim=2))
    a = (q * d ** -0.5) @ k.transpose(-2, -1) + table.to(dtype)[index.reshape(-1).long()].view(N, N, heads).permute(2, 0, 1)[None]
    if region is not None:
        ids = region.repeat(Wn // region.shape[0], 1)
        a = a + ((ids[:, :, None] != ids[:, None, :]).to(dtype) * -100.0)[:, None]
    return (a.softmax(-1) @ v).transpose(1, 2).reshape(Wn, N, heads * d)


@pytest.mark.parametrize("masked", [False, True], ids=["bias", "bias+mask"])
@pytest.mark.parametrize("case", [(98, 16, 4, 192), (98, 16, 4, 96), (3, 4, 2, 32), (1, 64, 1, 64)], ids=str)
def test_window_attention(case, masked):
    Wn, N, heads, d = case
    w = int(round(N ** 0.5))
    qkv = rnd(7400 + N + d, Wn, N, 3 * heads * d)
    table = rnd(7401 + N, (2 * w - 1) ** 2, heads)
    index = torch.from_numpy(fastvqa.relative_index((1, w, w)).astype(np.int32))
    region = None
    if masked and Wn == 98:                                                                    # the shifted 28 x 28 map's own regions, two samples
        region = torch.from_numpy(fastvqa.geometry((1, 28, 28), (1, 4, 4), (1, 1), True)["region"])
        assert tuple(region.shape) == (49, 16) and len(region.unique()) == 9
    elif masked:
        region = torch.randint(0, 3, (Wn, N), generator=torch.Generator().manual_seed(7402), dtype=torch.int32)
        region[0, 0], region[0, 1:] = 0, 1                                                     # token 0 alone in its region: every neighbour is masked out
    got = ops.window_attention_f32(qkv.to(DEV), heads, table.to(DEV), index.to(DEV), region=None if region is None else region.to(DEV))
    assert tuple(got.shape) == (Wn, N, heads * d) and bool(torch.isfinite(got).all())
    gate_check(f"window attention {case} masked {masked}", got, _window_ref(qkv, heads, table, index, region, F64),
               _window_ref(qkv, heads, table, index, region, F32))
    if masked and Wn != 98:                                                                    # ... so token 0 attends to itself alone
        assert float((got[0, 0].cpu() - qkv[0, 0, 2 * heads * d:]).abs().max()) < 1e-6
    half = Wn // 2                                                                             # the later windows alone: batch-independent
    sub = None if region is None else (region[half:] if region.shape[0] == Wn else region).to(DEV)
    assert torch.equal(ops.window_attention_f32(qkv[half:].contiguous().to(DEV), heads, table.to(DEV), index.to(DEV), region=sub), got[half:])


@pytest.mark.parametrize("stage", [0, 1], ids=["28x28x768", "28x28x384"])
def test_swin_layer_production(stage):
    name = f"swintransformer{stage + 1}"
    sd, W = part(name + ".")
    C = Q.CFG["dim"] >> stage
    x = rnd(7500 + stage, 2, 784, C)
    got = Q.swin_stage(W, x.to(DEV), stage, channel_rows=False)
    args = (sd, name, Q.CFG, Q.CFG["swin_heads"][stage])
    want64, want32 = R.swin_stage(x.double(), *args, F64, Q.SWIN_SCALE), R.swin_stage(x, *args, F32, Q.SWIN_SCALE)
    gate_check(f"{name}: one BasicLayer (shift 0, shift 2) with the scaled residual", got, want64, want32)
    rows = Q.swin_stage(W, x.to(DEV), stage, channel_rows=True)
    assert torch.equal(rows, got.transpose(1, 2))


# ---- 4. the stages at production width, two crops each ----------------------------------------------------------------------------------
def test_crops_and_tokens_bit_for_bit():
    cfg = T.TINY
    g = torch.Generator().manual_seed(7600)
    org = torch.from_numpy(Q.crop_origins(40, 48, 32, 4))

    def case(dev_view, host, what):
        want = R.crops(host, cfg, F32)                                                          # [N crops,3,32,32]
        got = ops.maniqa_crops_f32(dev_view, org.to(DEV), 32, 8).cpu()
        n = want.shape[0]
        assert tuple(got.shape) == (n * 16, 192), what
        assert torch.equal(got.view(n, 4, 4, 3, 8, 8), want.view(n, 3, 4, 8, 4, 8).permute(0, 2, 4, 1, 3, 5)), what

    u8 = torch.randint(0, 256, (2, 40, 48, 3), generator=g, dtype=torch.uint8)
    case(u8.to(DEV).permute(0, 3, 1, 2), u8, "u8 frames")
    f32 = torch.rand(2, 3, 40, 48, generator=g)
    case(f32.to(DEV), f32, "f32")
    case(f32.bfloat16().to(DEV), f32.bfloat16(), "bf16")
    case(f32[:, :1].to(DEV), f32[:, :1], "one channel")
    big = torch.rand(2, 45, 51, 3, generator=g)
    case(big.to(DEV)[:, 2:42, 1:49].permute(0, 3, 1, 2), big[:, 2:42, 1:49].permute(0, 3, 1, 2), "a cropped, permuted view")
    sd, W = tiny()
    emb = rnd(7601, 3 * 16, 64)
    got = ops.maniqa_tokens_f32(emb.to(DEV), W.params["cls"].to(DEV), W.params["pos"].to(DEV)).cpu()
    want = torch.cat([sd["vit.cls_token"].expand(3, -1, -1), emb.view(3, 16, 64)], 1) + sd["vit.pos_embed"]
    assert torch.equal(got, want)


def test_vit_block_and_hook_gather_production():
    sd, W = part("vit.blocks.0.")
    x = rnd(7700, 2, 785, 768)
    xd = x.to(DEV)
    got = Q.vit_block(W, xd, 0)
    assert got.data_ptr() == xd.data_ptr()
    gate_check("one ViT block at 2 x 785 x 768", got, R.vit_block(x.double(), sd, 0, 12, F64), R.vit_block(x, sd, 0, 12, F32))
    feat = torch.full((2, 4 * 768, 784), float("nan"), device=DEV)
    for slot in (2, 0, 3, 1):
        Q.hook_gather(xd if slot == 2 else (xd + slot), feat, slot)
    host = xd.cpu()
    want = torch.cat([(host if slot == 2 else host + slot)[:, 1:] for slot in range(4)], 2).transpose(1, 2)
    assert torch.equal(feat.cpu(), want)                                                        # the cls row left out, every slot in its place
    # mix_f32's other forms: the scaled sum, in place and transposed, bit for bit (two roundings)
    a, r = rnd(7701, 2, 37, 70).to(DEV), rnd(7702, 2, 37, 70).to(DEV)
    want = (0.8 * a + r)
    assert torch.equal(ops.mix_f32(a, r, 0.8), want) and torch.equal(ops.mix_f32(a, r, 0.8, transpose=True), want.transpose(1, 2))
    buf = a.clone()
    assert ops.mix_f32(buf, r, 0.8, out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, want)
    with pytest.raises(ValueError, match="must not alias an input under transpose"):
        ops.mix_f32(a[:, :, :37], transpose=True, out=a[:, :, :37])


@pytest.mark.parametrize("C", [3072, 768])
def test_tablock_production(C):
    name = "tablock1.0" if C == 3072 else "tablock2.1"
    sd, W = part(name + ".")
    x = rnd(7800 + C, 2, C, 784, scale=3.0)                          # rows a few units large, as the residual stream's: a softmax with a shape
    xd = x.to(DEV)
    got = Q.tablock(W, xd, name)
    assert got.data_ptr() == xd.data_ptr()
    probe = []
    want64 = R.tablock(x.double(), sd, name, F64, Q.TAB_RESHAPE_QUIRK, probe)
    peak = float(probe[0].max(-1).values.mean())
    print(f"TABlock C = {C}: mean row maximum of the softmax {peak:.4f} (uniform {1 / C:.5f})")
    assert 2.0 / C <= peak <= 0.9
    gate_check(f"TABlock at ({C}, 784), two crops", got, want64, R.tablock(x, sd, name, F32, Q.TAB_RESHAPE_QUIRK))


def test_tablock_without_the_quirk(monkeypatch):
    sd, W = part("tablock2.0.", cfg=T.TINY)
    x = rnd(7900, 3, 24, 16, scale=2.0)
    monkeypatch.setattr(Q, "TAB_RESHAPE_QUIRK", False)
    plain = Q.tablock(W, x.to(DEV), "tablock2.0")
    gate_check("TABlock (24, 16) with a plain transpose back", plain, R.tablock(x.double(), sd, "tablock2.0", F64, False),
               R.tablock(x, sd, "tablock2.0", F32, False))
    monkeypatch.setattr(Q, "TAB_RESHAPE_QUIRK", True)
    quirk = Q.tablock(W, x.to(DEV), "tablock2.0")
    gate_check("TABlock (24, 16) with the reshape quirk", quirk, R.tablock(x.double(), sd, "tablock2.0", F64, True),
               R.tablock(x, sd, "tablock2.0", F32, True))
    assert float((quirk - plain).abs().max()) > 0.1


def test_conv1_and_swintransformer1_production():
    sd, W = part("conv1.", "swintransformer1.")
    x = rnd(8000, 2, 3072, 784)
    tokens = Q.conv1x1(W, x.to(DEV), "conv1")
    assert tuple(tokens.shape) == (2, 784, 768)
    c64, c32 = R.conv1x1(x.double(), sd, "conv1", F64), R.conv1x1(x, sd, "conv1", F32)
    gate_check("conv1 as a GEMM with a transposed store", tokens, c64.transpose(1, 2), c32.transpose(1, 2))
    got = Q.swin_stage(W, tokens, 0, channel_rows=True)
    args = (sd, "swintransformer1", Q.CFG, 4)
    gate_check("conv1 + swintransformer1 -> channel rows", got, R.swin_stage(c64.transpose(1, 2), *args, F64, Q.SWIN_SCALE).transpose(1, 2),
               R.swin_stage(c32.transpose(1, 2), *args, F32, Q.SWIN_SCALE).transpose(1, 2))


def test_head_production():
    sd, W = part("fc_score.", "fc_weight.")
    x = rnd(8100, 4, 784, 384)                                                                  # two frames of two crops
    hidden = ops.linear_f32(x.view(-1, 384).to(DEV), W.params["head.hidden.weight"], W.params["head.hidden.bias"], relu=True).view(4, 784, 768)
    got = Q.head(W, hidden, 2)
    assert got.dtype == F64 and tuple(got.shape) == (2,)
    gate_check("the weighted head, two frames of two crops", got, R.head(x.double(), sd, F64).view(2, 2).mean(1),
               R.head(x, sd, F32).view(2, 2).mean(1))
    # the fp64 part alone, from the kernels' own hidden units: at rounding level of fp64
    h = hidden.cpu().double()
    f = torch.relu(h[..., :384] @ sd["fc_score.3.weight"].double().flatten() + sd["fc_score.3.bias"].double())
    w = torch.sigmoid(h[..., 384:] @ sd["fc_weight.3.weight"].double().flatten() + sd["fc_weight.3.bias"].double())
    want = ((f * w).sum(1) / w.sum(1)).view(2, 2).mean(1)
    assert float((got.cpu() - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- 5. the whole network on the tiny configuration -------------------------------------------------------------------------------------
def _tiny_ref(x):
    sd = T.state()
    return (R.maniqa(x, sd, T.TINY, F64, Q.TAB_RESHAPE_QUIRK, Q.SWIN_SCALE, Q.NUM_TAB),
            R.maniqa(x, sd, T.TINY, F32, Q.TAB_RESHAPE_QUIRK, Q.SWIN_SCALE, Q.NUM_TAB))


def test_tiny_network():
    sd, W = tiny()
    ref = T.reference()
    x = ref["x"]                                                                                # float32 [3,3,40,48]
    before = Q.COUNTERS["groups"]
    got = Q.maniqa(W, x.to(DEV))
    assert Q.COUNTERS["groups"] == before + 1 and got.dtype == F64 and tuple(got.shape) == (3,)
    gate_check("MANIQA tiny: float32, 3 channels", got, ref["s64"], ref["s32"])
    one = Q.maniqa(W, x.to(DEV), group=1)
    assert Q.COUNTERS["groups"] == before + 4 and torch.equal(one, got)                         # grouping 1 against the default
    assert torch.equal(Q.maniqa(W, x), got) and torch.equal(Q.maniqa(W, x.to(DEV), group=2), got)      # a host tensor; a ragged last group
    assert torch.equal(Q.ManiqaMetric(W)(x), got)
    u8 = (x * 255).round().to(torch.uint8)
    variants = {"uint8, 3 channels": u8, "uint8 frames [F,H,W,3]": u8.permute(0, 2, 3, 1).contiguous(), "uint8, 1 channel": u8[:, :1],
                "float32, 1 channel": x[:, 1:2], "bfloat16, 3 channels": x.bfloat16(), "bfloat16, 1 channel": x[:, 2:].bfloat16()}
    for what, v in variants.items():
        w64, w32 = _tiny_ref(v)
        g = Q.maniqa(W, v.to(DEV))
        gate_check(f"MANIQA tiny: {what}", g, w64, w32)
        assert torch.equal(Q.maniqa(W, v), g), what
    assert torch.equal(Q.maniqa(W, u8.permute(0, 2, 3, 1).contiguous()), Q.maniqa(W, u8))
    with pytest.raises(ValueError, match="too small"):
        Q.maniqa(W, torch.zeros(1, 3, 31, 48))


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setattr(Q, "CFG", T.TINY)                                 # the tool on the tiny network
    sd, _ = tiny()
    torch.save({"params": sd}, tmp_path / "maniqa_tiny.pth")
    pred = tmp_path / "pred"
    (pred / "png").mkdir(parents=True)
    g = torch.Generator().manual_seed(8200)
    frames = torch.randint(0, 256, (3, 40, 56, 3), generator=g, dtype=torch.uint8)
    for i, fr in enumerate(frames):
        Image.fromarray(fr.numpy()).save(pred / "png" / f"{i:04d}.png")
    clip = torch.randint(0, 256, (2, 36, 33, 3), generator=g, dtype=torch.uint8)
    np.save(pred / "clip.npy", clip.numpy())
    np.save(pred / "small.npy", np.zeros((2, 20, 40, 3), dtype=np.uint8))
    live = torch.cuda.memory_allocated()
    out = Q.main(["eval", "--pred", str(pred), "--metric_weights", str(tmp_path), "--out", str(tmp_path / "o")])
    W = Q.ManiqaWeights.load(str(tmp_path))
    want = {}
    for name in ("clip.npy", "png"):
        vals = Q.maniqa(W, prepost.load_frames(str(pred / name))).cpu().tolist()
        s = 0.0
        for v in vals:
            s += v
        want[name.split(".")[0]] = {"maniqa": round(s / len(vals), 4)}
    assert out["per_sample"] == want and out["count"] == 2 and want["clip"] != want["png"]
    with open(tmp_path / "o" / "metrics_maniqa.json") as f:
        assert json.load(f) == out
    (tmp_path / "img").mkdir()
    Image.fromarray(frames[1].numpy()).save(tmp_path / "img" / "a.png")
    scores = Q.main(["score", "--pred", str(tmp_path / "img"), "--metric_weights", str(tmp_path)])
    assert scores == {"a.png": float(Q.maniqa(W, frames[1:2])[0])}
    del W
    _drop_device_tables()
    gc.collect()
    assert torch.cuda.memory_allocated() <= live, "the tool left tensors on the device"
