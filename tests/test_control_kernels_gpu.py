"""The Wan-Fun control entries (include/vstyler_control.h), each against plain torch on the smallest shapes at
which it can go wrong: bit for bit, except the camera rays' values (fp32 arithmetic rounded to bf16: the bound
of funcontrol_util.RAY_SLACK)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import funcontrol_util as FU
import gpu_util as U

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def rand_bf16(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(BF16)


# ------------------------------------------------------------------------------------- vs_unpatchify_skip
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("HW", [(2, 2), (6, 10), (8, 12)])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("C", [16, 48])
def test_unpatchify_skip(C, T, HW, B):
    """Against slicing + the reference's rearrange 'b (f h w) (x y z c) -> b c (f x) (h y) (w z)'; skip 0
    against vs_unpatchify."""
    from vstyler import kernels as K
    H, W = HW
    h, w = H // 2, W // 2
    n, S = h * w, T * h * w
    for skip in sorted({0, 1, n, 3 * n}):
        tok = rand_bf16((B * (skip + S), 4 * C), seed=C + T + H + B + skip)
        want = tok.view(B, skip + S, 4 * C)[:, skip:].reshape(B, T, h, w, 2, 2, C).permute(0, 6, 1, 2, 4, 3, 5) \
            .reshape(B, C, T, H, W)
        got = K.unpatchify_skip(tok.cuda(), U.sentinel((B, C, T, H, W)), skip)
        assert torch.equal(U.bits(got.cpu()), U.bits(want.contiguous())), skip
        if skip == 0:
            plain = K.unpatchify(tok.cuda(), U.sentinel((B, C, T, H, W)))
            assert torch.equal(U.bits(got), U.bits(plain))
    with pytest.raises(ValueError):
        K.unpatchify_skip(tok.cuda(), U.sentinel((B, C, T, H, W)), 3 * n + 1)


# -------------------------------------------------------------------------------------------- vs_ref_rows
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S", [1, 72])
@pytest.mark.parametrize("n", [1, 24])
@pytest.mark.parametrize("D", [256, 1536, 5120])
def test_ref_rows_touches_only_the_reference_rows(D, n, S, B, per_sample):
    from vstyler import kernels as K
    src = rand_bf16(((B if per_sample else 1) * n, D), seed=D + n + S + B)
    dst = U.sentinel((B * (n + S), D))
    K.ref_rows(src.cuda(), dst, B, n, S)
    got = dst.cpu().view(B, n + S, D)
    assert U.untouched(got[:, n:])
    want = src.view(-1, n, D).expand(B, n, D)
    assert torch.equal(U.bits(got[:, :n]), U.bits(want.contiguous()))


# --------------------------------------------------------------------------------------- vs_camera_im2col
@pytest.mark.parametrize("HW", [(16, 16), (32, 48), (64, 96)])
@pytest.mark.parametrize("T", [1, 3])
def test_camera_im2col(T, HW):
    """Against torch: PixelUnshuffle(8), then the 2x2 / stride 2 unfold, rows in (t, oy, ox) order."""
    from vstyler import kernels as K
    H, W = HW
    C = 24
    x = rand_bf16((C, T, H, W), seed=T + H + W)
    un = F.pixel_unshuffle(x.permute(1, 0, 2, 3).float(), 8)                     # [T, 64 C, H/8, W/8]
    want = F.unfold(un, kernel_size=2, stride=2).transpose(1, 2).reshape(T * (H // 16) * (W // 16), 256 * C).to(BF16)
    rows = T * (H // 16) * (W // 16)
    buf = U.sentinel((rows + 2, 256 * C))
    got = K.camera_im2col(x.cuda(), buf[1:1 + rows])
    assert U.untouched(buf[:1]) and U.untouched(buf[1 + rows:])
    assert torch.equal(U.bits(got.cpu()), U.bits(want))


# ------------------------------------------------------------------------------------------------ vs_relu
def test_relu_every_bf16():
    """Every finite bf16 bit pattern (and the infinities) against torch.relu on the device."""
    from vstyler import kernels as K
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    finite = allb[~torch.isnan(allb.float())].contiguous()
    finite = finite[:finite.numel() // 8 * 8].cuda()
    want = torch.relu(finite.clone())
    got = K.relu(finite.clone())
    assert torch.equal(U.bits(got), U.bits(want))
    assert float(got.float().min()) == 0.0 and torch.equal(got[got > 0], finite[finite > 0])


# ----------------------------------------------------------------------------------------- vs_camera_rays
def _matrices(F_, H, W, seed):
    """Distinct intrinsics and poses per frame: rays that differ between any two frames."""
    g = np.random.default_rng(seed)
    intr = np.stack([np.array([0.9 * W + 3 * f, 1.1 * H + 2 * f, 0.5 * W + 0.25 * f, 0.5 * H - 0.5 * f]) for f in range(F_)])
    c2w = np.zeros((F_, 3, 4))
    for f in range(F_):
        q, _ = np.linalg.qr(g.standard_normal((3, 3)))
        c2w[f, :, :3], c2w[f, :, 3] = q, g.standard_normal(3)
    return intr.astype(np.float32), c2w.astype(np.float32)


def _rays(intr, c2w, T, H, W):
    from vstyler import kernels as K
    out = U.sentinel((24, T, H, W))
    K.camera_rays(torch.from_numpy(intr).cuda(), torch.from_numpy(c2w).cuda(), out)
    return out.cpu()


def _within(got, ref, tag):
    """|got - ref| <= 2^-8 |ref| + RAY_SLACK: bf16's half ulp of the float64 value plus what two correct fp32
    evaluations can differ by (funcontrol_util: measured 2.7 * 2^-24 between the reference's fp32 and the
    float64 restatement over the fixture cases and a 480x832 frame; slack = 4 x that = 10.8 * 2^-24)."""
    got, ref = got.double(), torch.as_tensor(ref).double()
    excess = (got - ref).abs() - (2.0 ** -8 * ref.abs() + FU.RAY_SLACK)
    print(f"{tag}: max |got - ref| {float((got - ref).abs().max()):.3g}, max excess over the bound {float(excess.max()):.3g}")
    assert float(excess.max()) <= 0, tag


@pytest.mark.parametrize("F_,HW", [(5, (16, 32)), (9, (48, 80))])
def test_camera_rays_grouping(F_, HW):
    """out[c 4 + j][t] is frame max(0, 4 t + j - 3)'s component c, exactly: every (t, j) slot against the
    kernel's own rays of that frame computed alone (a one-frame call puts frame 0 into all four slots)."""
    H, W = HW
    T = (F_ + 3) // 4
    intr, c2w = _matrices(F_, H, W, seed=F_)
    out = _rays(intr, c2w, T, H, W).view(6, 4, T, H, W)
    single = [_rays(intr[f:f + 1], c2w[f:f + 1], 1, H, W).view(6, 4, H, W) for f in range(F_)]
    for f in range(F_):
        assert all(torch.equal(U.bits(single[f][:, j]), U.bits(single[f][:, 0])) for j in range(4))
        for g in range(f):
            assert not torch.equal(U.bits(single[f][:, 0]), U.bits(single[g][:, 0]))
    for t in range(T):
        for j in range(4):
            assert torch.equal(U.bits(out[:, j, t]), U.bits(single[max(0, 4 * t + j - 3)][:, 0])), (t, j)


def test_camera_rays_values():
    """Against the float64 restatement (distinct frames, 9 frames at 48x80) and against the fixture -- the
    reference implementation's own fp32 output for the host path's matrices (5 frames at 16x32)."""
    from vstyler.camera import camera_matrices
    H, W, F_ = 48, 80, 9
    intr, c2w = _matrices(F_, H, W, seed=3)
    got = _rays(intr, c2w, 3, H, W)
    ref = FU.group_in_fours(torch.from_numpy(FU.plucker64(intr, c2w, H, W)), F_)[0]
    _within(got, ref, "9 frames 48x80 vs float64")
    for name, (direction, speed, origin, plucker) in FU.fixture().items():
        intr, c2w = camera_matrices(direction, 5, 16, 32, speed, origin)
        got = _rays(intr, c2w, 2, 16, 32)
        _within(got, FU.group_in_fours(torch.from_numpy(plucker), 5)[0], f"fixture {name} (reference fp32)")
        _within(got, FU.group_in_fours(torch.from_numpy(FU.plucker64(intr, c2w, 16, 32)), 5)[0], f"fixture {name} vs float64")
    assert float(got.view(6, 4, 2, 16, 32)[:3].float().abs().max()) > 0.05          # o x d is exercised
