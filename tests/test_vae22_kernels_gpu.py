"""The Wan2.2 VAE's kernels (include/vstyler_vae22.h, csrc/vae22.hip) one by one, and the existing kernels at the
widths only this model sends them: vs_vae_conv at every (cin, cout, kernel, stride, up2, split) of the real
configuration (dim 160, dec_dim 256) and the GEMM route of the attention block at 640 and 1024 channels.

Data movement (patchify, unpatchify, DupUp3D) and everything whose fp32 sums are exact (AvgDown3D on
k 2^-6 inputs, the convolutions on small integers) is held to the bit; AvgDown3D on random inputs to the
interval its fp32 sum can reach; the wide RMS norm to the bar of test_vae_gpu.py::test_rmsnorm_silu_bit_exact;
the attention block to the bar of test_vae_gpu.py::test_attention_block."""
import math

import pytest
import torch
import torch.nn.functional as F

import gpu_util as U
import vae22_util as U22
from oracle import wan_vae_oracle as V

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _vae():
    from vstyler import vae
    return vae


def _nthwc(x):
    """(B, C, T, H, W) -> (B, T, H, W, C) contiguous on the GPU."""
    return x.permute(0, 2, 3, 4, 1).contiguous().cuda()


def _ncthw(y):
    return y.cpu().permute(0, 4, 1, 2, 3)


# ------------------------------------------------------------------------------------------ patchify
@pytest.mark.parametrize("h,w", [(2, 2), (2, 10), (6, 2), (6, 10)])
@pytest.mark.parametrize("nt", [1, 5])
@pytest.mark.parametrize("ld", [4, 32])
def test_patchify_bit_exact(h, w, nt, ld):
    g = torch.Generator().manual_seed(h * 100 + w * 10 + nt + ld)
    src = torch.randn((nt, h, w, ld), generator=g).to(BF16)
    want = U22.patchify(src[..., :3].permute(3, 0, 1, 2)[None])[0].permute(1, 2, 3, 0)      # [nt, h/2, w/2, 12]
    dst = U.sentinel((nt + 1, h // 2, w // 2, 32))                                          # + a guard frame
    U.call("vs_vae22_patchify", src.cuda().data_ptr(), ld, dst.data_ptr(), nt, h, w, U.stream())
    torch.cuda.synchronize()
    assert U.same_bits(dst[:nt, ..., :12], want.contiguous())
    assert U.bit_zero(dst[:nt, ..., 12:]) and U.untouched(dst[nt])


@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (3, 1), (3, 5)])
@pytest.mark.parametrize("nt", [1, 5])
@pytest.mark.parametrize("ld", [12, 16, 32])
def test_unpatchify_bit_exact(h, w, nt, ld):
    g = torch.Generator().manual_seed(h * 100 + w * 10 + nt + ld)
    src = torch.randn((nt, h, w, ld), generator=g).to(BF16)
    want = U22.unpatchify(src[..., :12].permute(3, 0, 1, 2)[None])[0].permute(1, 2, 3, 0)   # [nt, 2h, 2w, 3]
    dst = U.sentinel((nt + 1, 2 * h, 2 * w, 4))
    U.call("vs_vae22_unpatchify", src.cuda().data_ptr(), ld, dst.data_ptr(), nt, h, w, U.stream())
    torch.cuda.synchronize()
    assert U.same_bits(dst[:nt, ..., :3], want.contiguous())
    assert U.bit_zero(dst[:nt, ..., 3]) and U.untouched(dst[nt])
    # and back: patchify of the result is the source's 12 channels
    back = U.sentinel((nt, h, w, 32))
    U.call("vs_vae22_patchify", dst.data_ptr(), 4, back.data_ptr(), nt, 2 * h, 2 * w, U.stream())
    assert U.same_bits(back[..., :12], src[..., :12].contiguous())


# ------------------------------------------------------------------------------------------- DupUp3D
@pytest.mark.parametrize("c_in,c_out,ft,fs,t_in", [(1024, 1024, 2, 2, 1), (1024, 1024, 2, 2, 3), (1024, 512, 2, 2, 1),
                                                   (1024, 512, 2, 2, 3), (512, 256, 1, 2, 1), (512, 256, 1, 2, 3),
                                                   (32, 32, 2, 2, 2), (32, 32, 1, 1, 2)])
def test_dupup_bit_exact(c_in, c_out, ft, fs, t_in):
    """y + DupUp3D(x) against torch: repeat_interleave + view + permute + the first-frame drop + a bf16 add,
    on a 2 x 3 grid, two samples; a guard sample behind y stays untouched."""
    vae = _vae()
    g = torch.Generator().manual_seed(c_in + c_out + 7 * t_in + ft)
    x = torch.randn((2, c_in, t_in, 2, 3), generator=g).to(BF16)
    t_out = ft * (t_in - 1) + 1
    y0 = torch.randn((2, c_out, t_out, 2 * fs, 3 * fs), generator=g).to(BF16)
    want = y0 + U22.dup_up(x, c_out, ft, fs)
    buf = U.sentinel((3, t_out, 2 * fs, 3 * fs, c_out))
    buf[:2] = _nthwc(y0)
    vae.dupup_add(_nthwc(x), buf[:2], ft, fs)
    torch.cuda.synchronize()
    assert U.same_bits(_ncthw(buf[:2]).contiguous(), want.contiguous())
    assert U.untouched(buf[2])


# ------------------------------------------------------------------------------------------ AvgDown3D
AVGDOWN_CASES = [(160, 160, 1, 2), (160, 320, 2, 2), (320, 640, 2, 2), (640, 640, 1, 1)]


def _avgdown_run(x, y0, c_out, ft, fs):
    vae = _vae()
    n, t_out, ho, wo = y0.shape[0], y0.shape[2], y0.shape[3], y0.shape[4]
    buf = U.sentinel((n + 1, t_out, ho, wo, c_out))
    buf[:n] = _nthwc(y0)
    vae.avgdown_add(_nthwc(x), buf[:n], ft, fs)
    torch.cuda.synchronize()
    assert U.untouched(buf[n])
    return _ncthw(buf[:n]).contiguous()


@pytest.mark.parametrize("c_in,c_out,ft,fs", AVGDOWN_CASES)
@pytest.mark.parametrize("t_in", [1, 5])
def test_avgdown_exact_sums(c_in, c_out, ft, fs, t_in):
    """Inputs k 2^-6 with |k| <= 256: every fp32 group sum is exact in any order (|sum| <= 2^12 2^-6 in units
    of 2^-6), so y + mean has one answer: torch's bf16 `y + x.mean(2)` on the folded tensor, the zero frame in
    front of a temporal block prepended by hand (vae22_util.avg_down)."""
    g = torch.Generator().manual_seed(c_in + c_out + t_in)
    x = (torch.randint(-256, 257, (2, c_in, t_in, 4, 6), generator=g).float() * 2.0 ** -6).to(BF16)
    assert torch.equal(x.float() * 64, (x.float() * 64).round())
    t_out = 1 + (t_in - 1) // 2 if ft == 2 else t_in
    y0 = torch.randn((2, c_out, t_out, 4 // fs, 6 // fs), generator=g).to(BF16)
    want = y0 + U22.avg_down(x, c_out, ft, fs)
    got = _avgdown_run(x, y0, c_out, ft, fs)
    assert U.same_bits(got, want.contiguous()), int((U.bits(got) != U.bits(want.contiguous())).sum())


@pytest.mark.parametrize("c_in,c_out,ft,fs", AVGDOWN_CASES)
def test_avgdown_random_within_fp32_sum(c_in, c_out, ft, fs):
    """Normal inputs: with m64 the float64 mean and e = g 2^-24 max|x| over the group (the fp32 summation
    error), every element lies between bf16(y + bf16(m64 - e)) and bf16(y + bf16(m64 + e)) -- both roundings
    are monotone."""
    g = torch.Generator().manual_seed(3 * c_in + c_out)
    t_in = 5
    x = torch.randn((2, c_in, t_in, 4, 6), generator=g).to(BF16)
    t_out = 1 + (t_in - 1) // 2 if ft == 2 else t_in
    y0 = torch.randn((2, c_out, t_out, 4 // fs, 6 // fs), generator=g).to(BF16)
    grp = c_in * ft * fs * fs // c_out
    m64 = U22.avg_down(x.double(), c_out, ft, fs)
    # max|x| over each group: the same folding, amax in place of the mean
    xa = F.pad(x.double().abs(), (0, 0, 0, 0, 1, 0)) if ft == 2 else x.double().abs()
    b, c, t, h, w = xa.shape
    xa = xa.reshape(b, c, t // ft, ft, h // fs, fs, w // fs, fs).permute(0, 1, 3, 5, 7, 2, 4, 6)
    e = grp * 2.0 ** -24 * xa.reshape(b, c_out, grp, t // ft, h // fs, w // fs).amax(dim=2)
    rb = lambda v: v.float().to(BF16)  # noqa: E731
    lo = rb(y0.double() + rb(m64 - e).double()).float()
    hi = rb(y0.double() + rb(m64 + e).double()).float()
    got = _avgdown_run(x, y0, c_out, ft, fs).float()
    bad = (got < lo) | (got > hi)
    print(f"avgdown {c_in}->{c_out}: {int((lo != hi).sum())} of {lo.numel()} intervals wider than a point")
    assert not bool(bad.any()), int(bad.sum())


# ------------------------------------------------------------------------------------- wide RMS norm
@pytest.mark.parametrize("c", [416, 640, 1024])
def test_wide_rmsnorm(c):
    """vs_vae22_rmsnorm (vae.rmsnorm above 384 channels) against the oracle's bf16 ops: <= 1 bf16 ulp and
    > 99.5 % bit-equal, with and without SiLU, out of place, in place, and with rows ldx > c apart."""
    vae = _vae()
    g = torch.Generator().manual_seed(c)
    x = (2.0 * torch.randn((3, c, 2, 5, 7), generator=g)).to(BF16)
    gamma = (1 + 0.1 * torch.randn((c, 1, 1, 1), generator=g)).to(BF16)
    gd = gamma.reshape(-1).cuda()
    npix = 3 * 2 * 5 * 7
    for silu in (False, True):
        ref = V.rms_norm(x, gamma)
        if silu:
            ref = F.silu(ref)

        def check(got, what):
            d = (got.float() - ref.float()).abs()
            ulp = ref.float().abs().clamp_min(1e-30) * 2.0 ** -7
            same = (got == ref).float().mean().item()
            print(f"rmsnorm c={c} silu={silu} {what}: max|d| {d.max().item():.3g}, bit-equal {same:.5f}")
            assert (d <= ulp).all(), (c, silu, what, d.max().item())
            assert same > 0.995, (c, silu, what, same)

        xg = _nthwc(x)
        check(_ncthw(vae.rmsnorm(xg, gd, silu)), "out of place")
        assert U.same_bits(xg, _nthwc(x))                                   # the input is not written
        check(_ncthw(vae.rmsnorm(xg, gd, silu, out=xg)), "in place")
        # rows ldx = c + 24, ldy = c + 8 apart, NaN between them and behind the last one
        xs, ys = U.sentinel((npix + 1, c + 24)), U.sentinel((npix + 1, c + 8))
        xs[:npix, :c] = _nthwc(x).reshape(npix, c)
        U.call("vs_vae22_rmsnorm", xs.data_ptr(), c + 24, ys.data_ptr(), c + 8, gd.data_ptr(), npix, c, int(silu),
               U.stream())
        torch.cuda.synchronize()
        assert U.untouched(ys[:npix, c:]) and U.untouched(ys[npix])
        check(_ncthw(ys[:npix, :c].reshape(3, 2, 5, 7, c)), "strided")


# ------------------------------------------------------------------- vs_vae_conv at the Wan2.2 widths
def _k3(cin, cout, res=True, real=None):
    return dict(cin=cin, cout=cout, k=(3, 3, 3), pad=(2, 1, 1), res=res, real=real)


def _k1(cin, cout, res=False, real=None, ldy=None):
    return dict(cin=cin, cout=cout, k=(1, 1, 1), res=res, real=real, ldy=ldy)


def _conv_cases():
    """Every distinct (cin, cout, kernel, stride, up2, split) of WanVideoVAE38(dim=160, dec_dim=256), by the
    layer that sends it.  real: the weight's input channels when the activation is padded to 32."""
    c = {"enc_conv1_12_160": _k3(32, 160, res=False, real=12), "enc_head_640_96": _k3(640, 96, res=False),
         "conv1_96_96": _k1(96, 96), "conv2_48_48": _k1(64, 48, real=48, ldy=64),
         "dec_conv1_48_1024": _k3(64, 1024, res=False, real=48),
         "dec_head_256_12": dict(_k3(256, 12, res=False), ldy=16)}
    for a, b in ((160, 160), (160, 320), (320, 320), (320, 640), (640, 640), (1024, 1024), (1024, 512), (512, 512),
                 (512, 256), (256, 256)):
        c[f"res_k3_{a}_{b}"] = _k3(a, b)                  # residual.2 / residual.6 (the latter with the residual)
    for a, b in ((160, 320), (320, 640), (1024, 512), (512, 256)):
        c[f"shortcut_{a}_{b}"] = _k1(a, b)
    for ch in (640, 1024):
        c[f"to_qkv_{ch}"] = _k1(ch, 3 * ch)
        c[f"proj_{ch}"] = _k1(ch, ch, res=True)
    for ch in (160, 320, 640):                            # Resample38 down: ZeroPad2d((0, 1, 0, 1)) + 3x3 stride 2
        c[f"down_{ch}"] = dict(cin=ch, cout=ch, k=(1, 3, 3), stride=(1, 2, 2), out=(3, 2, 3))
    for ch in (320, 640):                                 # downsample3d's time conv into frames 1..
        c[f"time_down_{ch}"] = dict(cin=ch, cout=ch, k=(3, 1, 1), stride=(2, 1, 1), out=(1, 4, 6), t_add=1, y_t=2)
    for ch in (1024, 512, 256):                           # Resample38 up: nearest x2 fused, the width kept
        c[f"up2_{ch}"] = dict(cin=ch, cout=ch, k=(1, 3, 3), pad=(0, 1, 1), up2=True, out=(3, 8, 12))
    for ch in (1024, 512):                                # upsample3d's time conv: frames 1.., halves -> frames
        c[f"time_up_{ch}"] = dict(cin=ch, cout=2 * ch, k=(3, 1, 1), pad=(1, 0, 0), out=(2, 4, 6), t_lo=1, t_mul=2,
                                  t_add=1, split=ch, y_t=5)
    return c


CONV_CASES = _conv_cases()
T_IN, H_IN, W_IN = 3, 4, 6


def _conv_problem(name):
    """Small-integer inputs whose fp32 sums are exact: x, w in {-1, 0, 1} at a density that keeps the sum of
    N = cin kt kh kw products near sqrt(N) d = 16, bias in -3..3, the residual in -8..8.  Every partial sum is
    an integer below 2^24 in any order, and bf16(acc + bias), bf16(that + res) are exact within +-256
    (asserted).  Returns CPU tensors and the answer per output frame."""
    c = CONV_CASES[name]
    cin, cout, (kt, kh, kw) = c["cin"], c["cout"], c["k"]
    real = c.get("real") or cin
    st, pad = c.get("stride", (1, 1, 1)), c.get("pad", (0, 0, 0))
    to, ho, wo = c.get("out", (T_IN, H_IN, W_IN))
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    d = min(1.0, 16.0 / math.sqrt(real * kt * kh * kw))

    def tern(shape):
        return torch.randint(-1, 2, shape, generator=g).float() * (torch.rand(shape, generator=g) < d)
    x = tern((1, T_IN, H_IN, W_IN, cin))
    x[..., real:] = 0
    w = tern((cout, real, kt, kh, kw))
    bias = torch.randint(-3, 4, (cout,), generator=g).float()
    xz = x[..., :real].permute(0, 4, 1, 2, 3).clone()
    xz[:, :, :c.get("t_lo", 0)] = 0
    if c.get("up2"):
        xz = xz.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    back = [max(0, (o - 1) * s + k - 1 - p - (i - 1)) for o, s, k, p, i in
            zip((to, ho, wo), st, (kt, kh, kw), pad, xz.shape[2:])]
    xz = F.pad(xz, (pad[2], back[2], pad[1], back[1], pad[0], back[0]))
    acc = F.conv3d(xz, w, None, stride=st)[:, :, :to, :ho, :wo]
    assert acc.shape[2:] == (to, ho, wo)
    r1 = acc + bias.view(1, -1, 1, 1, 1)
    assert float(r1.abs().max()) <= 256 and float((r1 != 0).float().mean()) > 0.5, (float(r1.abs().max()),)
    return c, x.to(BF16), w.to(BF16), bias.to(BF16), r1, (to, ho, wo), g


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_at_wan22_widths_exact(name):
    vae = _vae()
    c, x, w, bias, r1, (to, ho, wo), g = _conv_problem(name)
    cout, split = c["cout"], c.get("split", 0)
    width = split if split else cout
    ldy = c.get("ldy") or cout if not split else split
    y_t = c.get("y_t", to)
    buf = U.sentinel((1, y_t + 1, ho, wo, ldy))                          # one guard frame
    res = None
    want = U.sentinel((1, y_t + 1, ho, wo, ldy), device="cpu")
    if c.get("res"):
        rr = torch.randint(-8, 9, (1, to, ho, wo, cout), generator=g).float()
        r2 = r1.permute(0, 2, 3, 4, 1) + rr
        assert float(r2.abs().max()) <= 256
        res = rr.to(BF16).cuda()
    else:
        r2 = r1.permute(0, 2, 3, 4, 1)
    t_mul, t_add = c.get("t_mul", 1), c.get("t_add", 0)
    for f in range(to):
        for sub in range(2 if split else 1):
            want[:, f * t_mul + t_add + sub, ..., :width] = r2[:, f, ..., sub * width:(sub + 1) * width].to(BF16)
    cw = vae.ConvW(w, bias, "cuda")
    assert (cw.cin, cw.cout) == (c["cin"], cout)
    vae.conv(x.cuda(), cw, (to, ho, wo), stride=c.get("stride", (1, 1, 1)), pad=c.get("pad", (0, 0, 0)),
             up2=bool(c.get("up2")), t_lo=c.get("t_lo", 0), y=buf[:, :y_t], t_mul=t_mul, t_add=t_add, split=split,
             res=res)
    torch.cuda.synchronize()
    got = buf.cpu()
    bad = int((U.bits(got) != U.bits(want)).sum())
    assert bad == 0, f"{bad} of {want.numel()} values differ (written and guard elements together)"


# ------------------------------------------------------------------------------- the split softmax
@pytest.mark.parametrize("ncols,pad", [(1, 31), (6, 26), (24, 8), (65, 31), (1560, 8)])
def test_softmax_split(ncols, pad):
    """vs_vae22_softmax_split: hi + lo against the float64 softmax of the same fp32 scores.  Relative bound per
    element j, in units of 2^-24, with x = s - max: 256 for lo = bf16(p - hi) (bf16 rounds to within 2^-8
    relative: |p - hi| <= 2^-8 p, and lo to within 2^-8 of that: 2^-16), |x_j| for the rounding of the exponent's argument and sum_k p_k |x_k| for the same
    in the row sum, ncols for the fp32 sum, and 8 for two expf (2 ulp each), the reciprocal and the product.
    |lo| <= 2^-8 hi: hi is a bf16 nearest to the pair's sum.  Pad columns of both halves are +0; a guard row
    stays untouched."""
    rows, half = 37, ncols + pad
    g = torch.Generator().manual_seed(ncols)
    s = (3.0 * torch.randn((rows, ncols + 3), generator=g)).float()
    s[0, :ncols] = -30.0
    s[0, 0] = 30.0                                              # a one-hot row: tails of exp(-60), still normal in bf16
    x = s[:, :ncols].double() - s[:, :ncols].double().amax(dim=-1, keepdim=True)
    want = torch.softmax(s[:, :ncols].double(), dim=-1)
    out = U.sentinel((rows + 1, 2 * half))
    U.call("vs_vae22_softmax_split", s.cuda().data_ptr(), ncols + 3, out.data_ptr(), 2 * half, rows, ncols, U.stream())
    torch.cuda.synchronize()
    got = out.cpu()
    assert U.untouched(got[rows])
    assert U.bit_zero(got[:rows, ncols:half]) and U.bit_zero(got[:rows, half + ncols:])
    hi, lo = got[:rows, :ncols].double(), got[:rows, half:half + ncols].double()
    d = (hi + lo - want).abs()
    units = 256 + x.abs() + (want * x.abs()).sum(dim=-1, keepdim=True) + ncols + 8
    bound = want * units * 2.0 ** -24
    print(f"softmax_split ncols={ncols}: worst error / bound {(d / bound).max().item():.3f}")
    assert bool((d <= bound).all()), (d / bound).max().item()
    assert bool((hi > 0).all()) and bool((lo.abs() <= hi * 2.0 ** -8).all())
    assert bool(((hi + lo).sum(dim=-1) - 1).abs().max() < 1e-4)


# ------------------------------------------------------------------------------ the attention block
@pytest.mark.parametrize("c", [640, 1024])
def test_attention_block_wide(c):
    """WanVideoVAE38._attn_block (the GEMM route with split probabilities) on 2 frames of 4 x 6 tokens, at
    test_attention_block's bar.  Inputs N(0, 1/4): below 4 in magnitude, so that one bf16 ulp of the output (2^-6) is under the
    absolute bar and not at it."""
    vae = _vae()
    g = torch.Generator().manual_seed(c)
    rnd = lambda shape, s: (s * torch.randn(shape, generator=g)).to(BF16)  # noqa: E731
    W = {"a.norm.gamma": (1 + 0.1 * torch.randn((c, 1, 1), generator=g)).to(BF16),
         "a.to_qkv.weight": rnd((3 * c, c, 1, 1), 1 / math.sqrt(c)), "a.to_qkv.bias": rnd((3 * c,), 0.1),
         "a.proj.weight": rnd((c, c, 1, 1), 1 / math.sqrt(c)), "a.proj.bias": rnd((c,), 0.1)}
    x = rnd((1, c, 2, 4, 6), 0.5)
    ref = V.attention_block(x, W, "a.")
    m = vae.WanVideoVAE38(device="cuda")
    m.params = {"a.norm.gamma": W["a.norm.gamma"].reshape(-1).cuda()}
    m.cw = {"a.to_qkv.": vae.ConvW(W["a.to_qkv.weight"], W["a.to_qkv.bias"], "cuda"),
            "a.proj.": vae.ConvW(W["a.proj.weight"], W["a.proj.bias"], "cuda")}
    got = _ncthw(m._attn_block(_nthwc(x), "a."))
    mx, rel = U.err(got, ref)
    print(f"attention block c={c}: max|d| {mx:.3g}, rel-L2 {rel:.3g}")
    assert rel < 4e-3 and mx < 3e-2, (mx, rel)
