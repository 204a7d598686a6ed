"""Two modulation / gate rows per sample (include/vstyler_seg.h, vs_epilogue.seg_rows): row m of sample
b = m / rows_per_batch reads table row 2 b + ((m - b rows_per_batch) >= seg_rows).

Row kernels: vs_layernorm_modulate_seg / _fp8_seg are bit-identical to the plain entries called per
(sample, segment) row slice with that segment's modulation row; the fp8 form's bytes and scales equal
vs_quant_fp8_rows of the bf16 form.

Gate epilogue: integer-valued operands whose fp32 accumulation is exact (the construction of
test_kernels_gpu.py's exact GEMM tests; the fp8 scales are powers of two, so a fused or an unfused
multiply-add gives the same bits), against a torch restatement with the epilogue's bf16 rounding points,
bit for bit -- on every kernel the dispatch or the options can choose, with short segments (the per-row
epilogue) and long ones (the persistent 4-wave kernel's two cached gate rows)."""
import pytest
import torch

import gpu_util as U
from gpu_util import BF16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from vstyler import kernels
    return kernels


def gate_index(M, rpb, seg, device="cuda"):
    m = torch.arange(M, device=device)
    b = m // rpb
    return (2 * b + ((m - b * rpb) >= seg).long()) if seg else b


# ------------------------------------------------------------------------------------------- row kernels
def slices(B, rpb, seg):
    """(row range, modulation row) of every non-empty (sample, segment)."""
    out = []
    for b in range(B):
        s0 = min(seg, rpb)
        out.append((b * rpb, b * rpb + s0, 2 * b))
        if s0 < rpb:
            out.append((b * rpb + s0, (b + 1) * rpb, 2 * b + 1))
    return out


@pytest.mark.parametrize("dim", [8, 1536, 3072, 5120, 8192])
@pytest.mark.parametrize("seg", [1, 36, 37, 50])
def test_layernorm_modulate_seg_equals_plain_per_slice(K, dim, seg):
    """vs_layernorm_modulate_seg and vs_layernorm_modulate_fp8_seg, 3 samples of 37 rows, ldx / ldo > dim,
    an affine weight on one of the dims."""
    B, rpb = 3, 37
    M, pad = B * rpb, 16
    g = torch.Generator(device="cuda").manual_seed(100 + dim + seg)
    xb = torch.randn(M, dim + pad, device="cuda", generator=g).to(BF16)
    x = xb[:, :dim]
    mod = (0.5 * torch.randn(2 * B, 2, dim, device="cuda", generator=g)).to(BF16)
    aff = dim == 1536
    w = (1 + 0.1 * torch.randn(dim, device="cuda", generator=g)).to(BF16) if aff else None
    bb = (0.1 * torch.randn(dim, device="cuda", generator=g)).to(BF16) if aff else None
    kw = dict(shift=mod[:, 0], scale=mod[:, 1], mod_bstride=2 * dim, rows_per_batch=rpb, weight=w, bias=bb)
    out = U.sentinel((M, dim + pad))
    K.layernorm_modulate_seg(x, out[:, :dim], seg, 1e-6, **kw)
    ref = torch.empty(M, dim, dtype=BF16, device="cuda")
    for r0, r1, row in slices(B, rpb, seg):
        K.layernorm_modulate(x[r0:r1], ref[r0:r1], 1e-6, shift=mod[row:, 0], scale=mod[row:, 1], mod_bstride=2 * dim,
                             rows_per_batch=r1 - r0, weight=w, bias=bb)
    assert U.same_bits(out[:, :dim], ref)
    assert U.untouched(out[:, dim:])
    # the fp8 form: vs_quant_fp8_rows of the bf16 form's rows
    x8 = torch.zeros(M, dim + pad, dtype=torch.uint8, device="cuda")
    qs = torch.zeros(M, dtype=torch.float32, device="cuda")
    K.layernorm_modulate_fp8_seg(x, x8[:, :dim], qs, seg, 1e-6, **kw)
    r8 = torch.empty(M, dim, dtype=torch.uint8, device="cuda")
    rs = torch.empty(M, dtype=torch.float32, device="cuda")
    K.quant_fp8_rows(ref, r8, rs)
    assert torch.equal(x8[:, :dim], r8) and torch.equal(qs, rs)
    assert not x8[:, dim:].any()


def test_layernorm_modulate_seg_equal_rows_is_one_plain_call(K):
    B, rpb, dim = 3, 37, 3072
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(B * rpb, dim, device="cuda", generator=g).to(BF16)
    one = (0.5 * torch.randn(B, 1, 2, dim, device="cuda", generator=g)).to(BF16)
    two = one.expand(B, 2, 2, dim).contiguous().view(2 * B, 2, dim)
    out, ref = torch.empty_like(x), torch.empty_like(x)
    K.layernorm_modulate_seg(x, out, 5, 1e-6, shift=two[:, 0], scale=two[:, 1], mod_bstride=2 * dim, rows_per_batch=rpb)
    K.layernorm_modulate(x, ref, 1e-6, shift=one[:, 0, 0], scale=one[:, 0, 1], mod_bstride=2 * dim, rows_per_batch=rpb)
    assert U.same_bits(out, ref)


# ---------------------------------------------------------------------------------------- gate epilogue
def bf(t):
    return t.to(BF16).float()


def epilogue_ref(acc, bias, res, gate, gidx, hint, hint_scale):
    """bf16(res + bf16(gate * bf16(acc + bias))) [+ bf16(hint * s)], the rounding points of epilogue_store_w."""
    y = bf(acc + bias.float())
    v = res.float() + bf(gate.float()[gidx] * y)
    if hint is not None:
        v = bf(v) + bf(hint.float() * hint_scale)
    return v.to(BF16)


class Problem:
    def __init__(self, B, rpb, N, Kd, seed, k2=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        M = B * rpb

        def ints(lo, hi, *shape):
            return torch.randint(lo, hi + 1, shape, device="cuda", generator=g)
        self.B, self.rpb, self.M, self.N, self.Kd = B, rpb, M, N, Kd
        self.a, self.w = ints(-3, 3, M, Kd).to(BF16), ints(-3, 3, N, Kd).to(BF16)
        self.bias = ints(-8, 8, N).to(BF16)
        self.res = torch.randn(M, N, device="cuda", generator=g).to(BF16)
        self.hint = torch.randn(M, N, device="cuda", generator=g).to(BF16)
        # distinct gate rows: a wrong row cannot give the right bits
        self.gate2 = (0.25 * torch.randn(2 * B, N, device="cuda", generator=g)).to(BF16)
        self.gate1 = self.gate2[:B].contiguous()
        self.acc = self.a.float() @ self.w.float().t()          # exact: |sum| <= 9 K < 2^24
        self.a2 = self.w2 = None
        if k2:
            self.a2, self.w2 = ints(-2, 2, M, k2).to(BF16), ints(-2, 2, N, k2).to(BF16)
            self.acc2 = self.a2.float() @ self.w2.float().t()
        # fp8: the same integers as e4m3 bytes, power-of-two row / column scales
        self.a8 = self.a.to(torch.float8_e4m3fn).view(torch.uint8)
        self.w8 = self.w.to(torch.float8_e4m3fn).view(torch.uint8)
        self.sa = torch.tensor([0.5, 1.0, 2.0], device="cuda")[ints(0, 2, M)].contiguous()
        self.sw = torch.tensor([0.25, 0.5, 1.0], device="cuda")[ints(0, 2, N)].contiguous()

    def ref(self, seg, hint, acc):
        gate = self.gate2 if seg else self.gate1
        return epilogue_ref(acc, self.bias, self.res, gate, gate_index(self.M, self.rpb, seg),
                            self.hint if hint else None, 0.5)

    def epi(self, K, seg, hint):
        x = self.res.clone()
        kw = dict(epilogue=K.VS_EPI_GATE_RES, bias=self.bias, residual=x, gate=self.gate2 if seg else self.gate1,
                  gate_bstride=self.N, rows_per_batch=self.rpb, seg_rows=seg)
        if hint:
            kw.update(hint=self.hint, hint_scale=0.5)
        return x, kw


@pytest.fixture(scope="module")
def big():
    """2 samples of 1928 rows (the sample boundary mid-tile), N 4096, K 1024: 16 x 16 tiles of 256 x 256, the
    persistent 4-wave route."""
    return Problem(2, 1928, 4096, 1024, seed=90, k2=64)


@pytest.fixture(scope="module")
def small():
    """2 samples of 200 rows, N 256, K 64: the 128 x 128 route."""
    return Problem(2, 200, 256, 64, seed=91)


BIG_SEGS = [0, 1, 127, 128, 129, 1000, 1927, 1928]
ROUTES = {"default": {}, "tile128": dict(gemm_tile=128), "8p": dict(gemm_tile=256, gemm_kernel=8),
          "4w_lists": dict(gemm_tile=256, gemm_kernel=4, queue=0), "4w_nosplit": dict(gemm_kernel=4, gemm_split=0)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("hint", [False, True])
def test_gemm_gate_seg_exact(K, opt, big, route, hint):
    opt(**ROUTES[route])
    for seg in BIG_SEGS:
        x, kw = big.epi(K, seg, hint)
        K.gemm(big.a, big.w, x, **kw)
        assert torch.equal(x, big.ref(seg, hint, big.acc)), (route, hint, seg)


@pytest.mark.parametrize("route", ["default", "8p"])
def test_gemm_gate_seg_lora_phase_exact(K, opt, big, route):
    opt(**ROUTES[route])
    for seg in BIG_SEGS:
        x, kw = big.epi(K, seg, True)
        K.gemm(big.a, big.w, x, a2=big.a2, w2=big.w2, **kw)
        assert torch.equal(x, big.ref(seg, True, big.acc + big.acc2)), (route, seg)


@pytest.mark.parametrize("route", ["default", "8p", "tile256_4w"])
@pytest.mark.parametrize("hint", [False, True])
def test_gemm_gate_seg_small_exact(K, opt, small, route, hint):
    opt(**dict(ROUTES, tile256_4w=dict(gemm_tile=256, gemm_kernel=4))[route])
    for seg in (0, 1, 199):
        x, kw = small.epi(K, seg, hint)
        K.gemm(small.a, small.w, x, **kw)
        assert torch.equal(x, small.ref(seg, hint, small.acc)), (route, hint, seg)


@pytest.mark.parametrize("form", ["fp8", "lora", "ws", "ws_lora"])
@pytest.mark.parametrize("kern", [4, 8])
def test_gemm_fp8_gate_seg_exact(K, opt, big, form, kern):
    """vs_gemm_fp8 (both 256 x 256 kernels), vs_gemm_fp8_lora and vs_gemm_fp8_ws (the 8-phase kernel whatever
    the option says)."""
    opt(gemm_kernel=kern)
    p = big
    acc = p.acc * p.sw[None, :] if form.startswith("ws") else p.acc
    acc = acc * p.sa[:, None]
    extra = {}
    if form.endswith("lora"):
        acc = acc + p.acc2
        extra.update(a2=p.a2, w2=p.w2)
    if form.startswith("ws"):
        extra.update(scale_w=p.sw)
    for hint in (False, True):
        for seg in BIG_SEGS:
            x, kw = p.epi(K, seg, hint)
            K.gemm_fp8(p.a8, p.sa, p.w8, x, **kw, **extra)
            assert torch.equal(x, p.ref(seg, hint, acc)), (form, kern, hint, seg)


@pytest.fixture(scope="module")
def tailed():
    """2 samples of 2056 rows, N 4096, K 2048: 17 x 16 tiles, one M-tile past a full round of 256 -- on 256
    CUs the plan is 256 whole tiles + 16 tail tiles (rows 4096-4111) as 4 K pieces, finished by
    gemm_split_combine."""
    return Problem(2, 2056, 4096, 2048, seed=92)


@pytest.mark.parametrize("route", ["default", "8p"])
def test_gemm_gate_seg_split_tail_combine_exact(K, opt, tailed, route):
    """The split-tail combine applies the epilogue of the tail tiles: seg_rows 1000 puts their rows in gate
    row 3 (row 1 if the combine ignored the segment), 2048 puts the segment boundary inside them (and,
    the second segment being 8 rows, sends the launch to the 8-phase kernel, whose tail is combined too);
    bf16 and fp8."""
    p = tailed
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus == 256:
        assert K.gemm_split_plan(p.M, p.N, p.Kd, cus) == (256, 16, 4, 512)
    opt(**ROUTES[route])
    acc8 = p.acc * p.sa[:, None]
    for hint in (False, True):
        for seg in (0, 1000, 2048):
            x, kw = p.epi(K, seg, hint)
            K.gemm(p.a, p.w, x, **kw)
            assert torch.equal(x, p.ref(seg, hint, p.acc)), (route, hint, seg)
            x, kw = p.epi(K, seg, hint)
            K.gemm_fp8(p.a8, p.sa, p.w8, x, **kw)
            assert torch.equal(x, p.ref(seg, hint, acc8)), ("fp8", route, hint, seg)
