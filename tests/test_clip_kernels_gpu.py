"""vs_clip_preprocess (include/vstyler_clip.h) on the GPU against tests/clip_util.py: bit for bit where
every step of the interpolation is exact in fp32, and inside the interval the fp32 evaluation's error
bound allows on real frames."""
import pytest
import torch
import torch.nn.functional as F

import clip_util as C
import gpu_util as G

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.mark.parametrize("size", C.EXACT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_clip_preprocess_exact(size):
    """Source sizes 224 m, pixel values k / 64: the answer is known to the bit.  n = 2 images read in place
    from a buffer with image, channel and row strides of its own; ld = 648 with two extra rows: the pad
    columns [588, 648) come out +0 and the extra rows keep their sentinel."""
    H, W = size
    u = C.exact_image(2, H, W, seed=3)
    want = C.im2col(C.preprocess(u))
    big = G.sentinel((2, 3, H + 1, W + 8))
    imgs = big[:, :, :H, :W]
    imgs.copy_(u)
    ld = 648
    tok = G.sentinel((2 * 256 + 2, ld))
    G.call("vs_clip_preprocess", imgs.data_ptr(), imgs.stride(0), imgs.stride(1), imgs.stride(2), tok.data_ptr(), ld,
           2, H, W, 224, G.stream())
    torch.cuda.synchronize()
    assert G.same_bits(tok[:512, :588].contiguous(), want)
    assert G.bit_zero(tok[:512, 588:]) and G.untouched(tok[512:])
    # one image repeated (image stride 0 is what the wrapper passes for n = 1), a contiguous ld = 640 buffer
    from vstyler.clip import clip_preprocess
    tok1 = clip_preprocess(imgs[1:], G.sentinel((256, 640)))
    assert G.same_bits(tok1[:, :588].contiguous(), want[256:]) and G.bit_zero(tok1[:, 588:])


def test_clip_preprocess_other_output_size():
    """out_size 56 (the 17-token tiny tower): 4 x 4 patches per image, same contract."""
    u = C.exact_image(2, 112, 56, seed=4)
    want = C.im2col(C.preprocess(u, 56))
    from vstyler.clip import clip_preprocess
    tok = G.sentinel((2 * 16 + 1, 640))
    clip_preprocess(u.cuda(), tok[:32], 56)
    assert G.same_bits(tok[:32, :588].contiguous(), want) and G.bit_zero(tok[:32, 588:]) and G.untouched(tok[32:])


@pytest.mark.parametrize("case", range(len(C.INTERVAL_SIZES)), ids=lambda i: "x".join(map(str, C.INTERVAL_SIZES[i])))
def test_clip_preprocess_interval(case):
    """Seeded u8 frames through preprocess_video, read in place as the pipeline does.  With r the float64
    interpolated value and delta = 2^-18 (first-order fp32 error of the 16-tap evaluation, sum |w| ~ 1.4 per
    axis, |pixel| <= 1: ~1.4e-6; an fp32 emulation measured 2.1e-6 worst), every output lies in
    [rest(r - delta), rest(r + delta)], rest = the five bf16 roundings (monotone).  The condition on the
    inputs -- the interval holds more than one value on at most 0.5 % of the elements -- is asserted from the
    reference alone.  Printed, not asserted: how far torch's own device F.interpolate path (coordinate
    scale*(o + 0.5) - 0.5 in fp32) is from the kernel's exact-rational coordinate."""
    from vstyler.clip import clip_preprocess
    from vstyler.vae import preprocess_video
    H, W = C.INTERVAL_SIZES[case]
    u8 = C.u8_image(H, W, 40 + case)
    frame = preprocess_video(u8.cuda())                      # (1, 3, 1, H, W)
    view = frame[:, :, 0]
    u = view.cpu()
    assert G.same_bits(u.contiguous(), C.frame_of_u8(u8))
    lo, hi = C.interval(u)
    wide = (G.bits(lo) != G.bits(hi)).double().mean().item()
    assert wide <= C.MAX_WIDE, wide
    got = clip_preprocess(view, G.sentinel((256, 640)))[:, :588].cpu()
    lo, hi = C.im2col(lo), C.im2col(hi)
    inside = (got >= lo) & (got <= hi)
    mid = C.im2col(C.preprocess(u))
    off = (G.bits(got) != G.bits(mid)).sum().item()
    dev_interp = F.interpolate(view, size=(224, 224), mode="bicubic", align_corners=False).cpu()
    t = C.im2col(C.rest(dev_interp))
    differ = G.bits(got) != G.bits(t)
    dmax = (got.double() - t.double()).abs().max().item()
    dev32 = F.interpolate(view.float(), size=(224, 224), mode="bicubic", align_corners=False).cpu()
    rmax = (dev32.double() - C.interp64(u)).abs().max().item()
    print(f"{H}x{W}: interval wider than one value on {100 * wide:.3f} %; outside it {int((~inside).sum())}; "
          f"off the float64 restatement {off} of {got.numel()}; against torch's device path: "
          f"{int(differ.sum())} elements differ ({100 * differ.double().mean().item():.3f} %), max |diff| {dmax:.4g} "
          f"after the roundings; torch's fp32 interpolated value is off the float64 one by up to {rmax:.3g}")
    assert bool(inside.all()), int((~inside).sum())
