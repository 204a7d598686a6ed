"""The four kernels of include/vstyler_motion.h, each alone (K.motion_stem, K.lrelu_blur, K.lrelu_merge,
K.motion_direction), against the torch expressions of the reference evaluated on the device and float64 sums
rounded once.

ACT(x, b) is the reference's `F.leaky_relu(x + b, 0.2) * 2**0.5` on bf16 tensors; the ResBlock tail is
`(out + skip) / math.sqrt(2)`.  Both are elementwise: bit for bit.  Where a kernel sums in fp32 (the blur's 16
taps, the stem's 3 terms, Direction's m products) two tiers: integer inputs, where every partial sum is exact and
the result must equal float64-then-round to the bit; and random normal inputs, equal bits except where the float64
value lies within 2^-20 relative of a bf16 rounding midpoint, a share of at most 0.1 % (motion_util
same_or_ambiguous)."""
import math

import pytest
import torch
import torch.nn.functional as F

import gpu_util as U
import motion_util as M

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def act_t(x, bias):
    """fused_leaky_relu on the device, channels-last: bias broadcasts over the last dim."""
    return F.leaky_relu(x + bias, 0.2) * 2 ** 0.5


def padded(t, extra=8):
    """A device copy of channels-last t [n, H, W, C] inside rows of C + extra, NaN sentinels between."""
    n, h, w, c = t.shape
    buf = U.sentinel((n, h, w, c + extra))
    buf[..., :c] = t.to(BF16).cuda()
    return buf, buf[..., :c]


# ------------------------------------------------------------------------------------------ vs_lrelu_merge
def test_act_every_bf16():
    """ACT over every finite bf16 value x 8 biases, bit for bit; rows at ld > C; in place equals out of place."""
    from vstyler import kernels as K
    v = M.all_finite_bf16()
    bias = torch.tensor([0.0, -0.0, 0.5, -0.1337, 3.0, -300.0, 1e-3, 2.0 ** 100]).to(BF16).cuda()
    x = v.view(1, 1, -1, 1).expand(1, 1, v.numel(), 8)
    buf, xv = padded(x)
    want = act_t(xv, bias)
    obuf = U.sentinel(tuple(buf.shape))
    got = K.lrelu_merge(xv, bias, out=obuf[..., :8])
    torch.cuda.synchronize()
    assert torch.equal(U.bits(got), U.bits(want))
    assert U.untouched(obuf[..., 8:])
    K.lrelu_merge(xv, bias)                                                 # in place
    torch.cuda.synchronize()
    assert torch.equal(U.bits(xv), U.bits(want)) and U.untouched(buf[..., 8:])


def test_merge_tail_every_bf16_and_pairs():
    """r(r(y + skip) / sqrt(2)) against `(y + skip) / math.sqrt(2)` on the device, bit for bit.  y is ACT's
    output, so it cannot be set directly: (1) x over every finite bf16 value with bias 0 and skip 0 -- y over the
    whole image of ACT; (2) x = 0, bias = 0 (y = 0) and skip over every finite bf16 value -- the sum y + skip, and
    with it the scaling, over every finite bf16 value; (3) random pairs with a bias, n = 2 frames, rows at ld > C,
    in place equal to out of place."""
    from vstyler import kernels as K
    v = M.all_finite_bf16().view(1, 1, -1, 8).cuda()
    zero = torch.zeros_like(v)
    b0 = torch.zeros(8, dtype=BF16, device="cuda")
    for x, skip in ((v, zero), (zero, v)):
        want = (act_t(x, b0) + skip) / math.sqrt(2)
        got = K.lrelu_merge(x, b0, skip, out=torch.empty_like(x))
        torch.cuda.synchronize()
        assert torch.equal(U.bits(got), U.bits(want))
    g = torch.Generator().manual_seed(3)
    x = 2 * torch.randn((2, 5, 7, 40), generator=g)
    skip = torch.randn((2, 5, 7, 40), generator=g)
    bias = (0.1 * torch.randn(40, generator=g)).to(BF16).cuda()
    xb, xv = padded(x)
    sb, sv = padded(skip, 16)
    want = (act_t(xv, bias) + sv) / math.sqrt(2)
    ob = U.sentinel(tuple(xb.shape))
    got = K.lrelu_merge(xv, bias, sv, out=ob[..., :40])
    torch.cuda.synchronize()
    assert torch.equal(U.bits(got), U.bits(want)) and U.untouched(ob[..., 40:])
    K.lrelu_merge(xv, bias, sv)
    torch.cuda.synchronize()
    assert torch.equal(U.bits(xv), U.bits(want)) and U.untouched(xb[..., 40:])


# ------------------------------------------------------------------------------------------- vs_lrelu_blur
SHAPES = [(4, 4), (5, 7), (8, 8), (33, 35)]
SETTINGS = [((2, 2), 1), ((1, 1), 2)]


def _border(t):
    m = torch.zeros(t.shape[1:3], dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def _run_blur(x, bias, pad, step):
    from vstyler import kernels as K
    n, h, w, c = x.shape
    ho, wo = -(-(h + sum(pad) - 3) // step), -(-(w + sum(pad) - 3) // step)
    xb, xv = padded(x)
    before = U.bits(xb).clone()
    ob = U.sentinel((n, ho, wo, c + 8))
    got = K.lrelu_blur(xv, ob[..., :c], bias, pad, step)
    torch.cuda.synchronize()
    assert torch.equal(U.bits(xb), before)
    assert U.untouched(ob[..., c:]), "pad channels touched"
    a = None if bias is None else act_t(xv, bias).cpu()             # the activation by torch on the device
    return got.cpu(), M.blur_ref64(x.to(BF16), a, pad[0], pad[1], step)


@pytest.mark.parametrize("hw", SHAPES)
def test_blur_exact(hw):
    """Integers in [-128, 128] (and integer biases): every fp32 partial sum is exact -- with ACT too, whose
    outputs are then multiples of 2^-9 below 2^9 -- so the bits equal float64-then-round.  Border rows and columns
    apart from the interior, so a wrong pad shows as such."""
    for c in (8, 32, 40):
        g = torch.Generator().manual_seed(hw[0] * 100 + c)
        x = torch.randint(-128, 129, (2, hw[0], hw[1], c), generator=g).float()
        ibias = torch.randint(-3, 4, (c,), generator=g).to(BF16).cuda()
        for pad, step in SETTINGS:
            for bias in (None, ibias):
                got, r64 = _run_blur(x, bias, pad, step)
                want = r64.to(BF16)
                tag = f"{hw} c={c} pad={pad} step={step} act={bias is not None}"
                assert got.shape == want.shape, tag
                eq = (got.float() == want.float())
                b = _border(got)
                assert bool(eq[:, ~b].all()), tag + f": {int((~eq[:, ~b]).sum())} interior elements differ"
                assert bool(eq[:, b].all()), tag + f": {int((~eq[:, b]).sum())} border elements differ"


@pytest.mark.parametrize("hw", SHAPES)
def test_blur_random(hw):
    for c in (8, 32, 40):
        g = torch.Generator().manual_seed(hw[0] * 1000 + c)
        x = torch.randn((2, hw[0], hw[1], c), generator=g)
        rbias = (0.1 * torch.randn(c, generator=g)).to(BF16).cuda()
        for pad, step in SETTINGS:
            for bias in (None, rbias):
                got, r64 = _run_blur(x, bias, pad, step)
                tag = f"{hw} c={c} pad={pad} step={step} act={bias is not None}"
                b = _border(got)
                M.same_or_ambiguous(got[:, ~b], r64[:, ~b], tag + " interior")
                M.same_or_ambiguous(got[:, b], r64[:, b], tag + " border")


def test_blur_other_pads():
    """Every (p0, p1) in 0..3 at both steps that leaves an output, against the same reference."""
    g = torch.Generator().manual_seed(9)
    x = torch.randint(-128, 129, (1, 6, 5, 8), generator=g).float()
    for p0 in range(4):
        for p1 in range(4):
            for step in (1, 2):
                got, r64 = _run_blur(x, None, (p0, p1), step)
                assert torch.equal(got.float(), r64.to(BF16).float()), (p0, p1, step)


# ------------------------------------------------------------------------------------------ vs_motion_stem
def _stem(frames, w, bias, n, h, wd):
    from vstyler import kernels as K
    c0 = w.shape[0]
    ob = U.sentinel((n, h, wd, c0 + 8))
    got = K.motion_stem(frames, w, bias, ob[..., :c0])
    torch.cuda.synchronize()
    assert U.untouched(ob[..., c0:])
    return got


def test_stem_every_byte():
    """All 256 byte values through px = r(r(u8 * (2 / 255)) + -1): channel k of a unit weight is ACT(px_k, 0),
    bit for bit against torch on the device; the uint8 and the planar bf16 input give identical bits."""
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1)
    u8 = torch.cat([u8, u8.flip(1), u8.transpose(1, 2)], dim=3).contiguous().cuda()         # [1, 16, 16, 3]
    u8 = torch.cat([u8, u8.flip(2)], dim=0).contiguous()                                    # n = 2
    w = torch.zeros(8, 3)
    w[0, 0] = w[1, 1] = w[2, 2] = 1.0
    w[3] = torch.tensor([1.0, 2.0, -1.0])
    w = w.to(BF16).cuda()
    bias = torch.tensor([0, 0, 0, 0.5, 0, 0, 0, -1.0]).to(BF16).cuda()
    px = u8.float().to(BF16) * (2 / 255) + -1                                               # [2, 16, 16, 3]
    assert px.min().item() == -1.0 and px.max().item() == 1.0
    got = _stem(u8, w, bias, 2, 16, 16)
    c = torch.stack([px[..., 0], px[..., 1], px[..., 2], (px[..., 0].double() + 2 * px[..., 1].double() -
                                                          px[..., 2].double()).to(BF16)] +
                    [torch.zeros_like(px[..., 0])] * 4, dim=-1)                             # (sums of 9-bit values: exact)
    want = act_t(c, bias)
    assert torch.equal(U.bits(got), U.bits(want))
    planar = px.permute(3, 0, 1, 2).contiguous()
    assert torch.equal(U.bits(_stem(planar, w, bias, 2, 16, 16)), U.bits(got))


def test_stem_sum():
    """The 3-term sum: integer pixels and weights bit for bit; normal ones within the midpoint exception."""
    g = torch.Generator().manual_seed(17)
    for exact in (True, False):
        if exact:
            px = torch.randint(-128, 129, (3, 2, 9, 11), generator=g).float()
            w = torch.randint(-3, 4, (32, 3), generator=g).float()
            bias = torch.randint(-3, 4, (32,), generator=g).float()
        else:
            px = torch.randn((3, 2, 33, 35), generator=g)
            w, bias = torch.randn((32, 3), generator=g), 0.1 * torch.randn(32, generator=g)
        px, w, bias = px.to(BF16), w.to(BF16), bias.to(BF16)
        got = _stem(px.cuda(), w.cuda(), bias.cuda(), 2, px.shape[2], px.shape[3]).cpu()
        c64 = torch.einsum("knhw,ck->nhwc", px.double(), w.double())
        want = act_t(c64.to(BF16).cuda(), bias.cuda()).cpu()
        diff = U.bits(got) != U.bits(want)
        amb = M.near_midpoint_rel(c64)
        print(f"stem sum exact={exact}: {int(diff.sum())} of {diff.numel()} differ, {int((diff & ~amb).sum())} outside "
              f"the midpoint window")
        if exact:
            assert not bool(diff.any())
        else:
            assert not bool((diff & ~amb).any()) and int(diff.sum()) <= 1e-3 * diff.numel()


# ------------------------------------------------------------------------------------- vs_motion_direction
def test_direction():
    """T in {1, 3}, m = 20 against r(sum_i r(alpha_i q_ji)): the products are exact roundings (rows with a single
    non-zero alpha return them alone, bit for bit); the sum by the two tiers."""
    from vstyler import kernels as K
    g = torch.Generator().manual_seed(23)
    q = torch.linalg.qr(torch.randn(512, 20, generator=g))[0].to(BF16).contiguous()     # (qr returns column-major)
    qi = torch.randint(-8, 9, (512, 20), generator=g).to(BF16)
    for T in (1, 3):
        abuf = U.sentinel((T, 32))
        alpha = torch.randn((T, 20), generator=g).to(BF16)
        abuf[:, :20] = alpha.cuda()
        got = K.motion_direction(abuf[:, :20], q.cuda(), torch.empty((T, 512), dtype=BF16, device="cuda")).cpu()
        prod = (alpha.float()[:, None, :] * q.float()[None]).to(BF16)
        M.same_or_ambiguous(got, prod.double().sum(-1), f"direction T={T}")
        ai = torch.randint(-8, 9, (T, 20), generator=g).to(BF16)
        got = K.motion_direction(ai.cuda(), qi.cuda(), torch.empty((T, 512), dtype=BF16, device="cuda")).cpu()
        assert torch.equal(got.float(), (ai.double() @ qi.double().t()).to(BF16).float())
    single = torch.diag(torch.randn(20, generator=g)).to(BF16)                              # row t: alpha_t e_t
    got = K.motion_direction(single.cuda(), q.cuda(), torch.empty((20, 512), dtype=BF16, device="cuda")).cpu()
    want = (single.float().diagonal()[:, None] * q.float().t()).to(BF16)
    assert torch.equal(got.float(), want.float())
