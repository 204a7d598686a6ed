"""Test-side restatement of Wan2.2-Animate's motion encoder (diffsynth/models/wan_video_animate_adapter.py:
321-612, Generator.get_motion) with the rounding points of include/vstyler_motion.h, its seeded weights, and the
references of the four kernels of that header.  Everything runs on CPU tensors.  Never used by the product path.

Two modes.  bf16 (default): every tensor the reference's bf16 modules materialise is rounded -- the elementwise
steps are the reference's own torch expressions on bf16 tensors, a convolution / linear accumulates in fp32 and
rounds once, the blur sums in float64 and rounds once.  PURE: float64 throughout, no rounding -- the arithmetic
of the float64 reference that tests/golden/make_motion_ref.py records."""
import math

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
PREFIX = "motion_encoder."
CHANNELS = {4: 512, 8: 512, 16: 512, 32: 512, 64: 256, 128: 128, 256: 64, 512: 32}
S2 = 2 ** 0.5
PURE = False


def pure_float64(fn):
    global PURE
    old, PURE = PURE, True
    try:
        return fn()
    finally:
        PURE = old


# ------------------------------------------------------------------------------------------------- weights
def motion_shapes(size, motion_dim=20):
    """The 63 tensors (at size 512) of Generator(size, 512, motion_dim) under the reference's names."""
    p = "enc.net_app.convs."
    c = CHANNELS[size]
    s = {p + "0.0.weight": (c, 3, 1, 1), p + "0.1.bias": (1, c, 1, 1)}
    n = 1
    for i in range(int(math.log2(size)), 2, -1):
        co = CHANNELS[2 ** (i - 1)]
        b = f"{p}{n}."
        s[b + "conv1.0.weight"], s[b + "conv1.1.bias"] = (c, c, 3, 3), (1, c, 1, 1)
        s[b + "conv2.0.kernel"], s[b + "conv2.1.weight"], s[b + "conv2.2.bias"] = (4, 4), (co, c, 3, 3), (1, co, 1, 1)
        s[b + "skip.0.kernel"], s[b + "skip.1.weight"] = (4, 4), (co, c, 1, 1)
        c, n = co, n + 1
    s[f"{p}{n}.weight"] = (512, c, 4, 4)
    for i in range(5):
        o = 512 if i < 4 else motion_dim
        s[f"enc.fc.{i}.weight"], s[f"enc.fc.{i}.bias"] = (o, 512), (o,)
    s["dec.direction.weight"] = (512, motion_dim)
    return s


def blur_kernel():
    k = torch.tensor([1.0, 3.0, 3.0, 1.0])
    k = k[None, :] * k[:, None]
    return k / k.sum()


def motion_weights(size, seed=41):
    """Seeded bf16-valued fp32 tensors under `motion_encoder.`: weights N(0, 1) (the reference's init; the
    equalised scale is applied at run time), biases 0.1 N(0, 1) (non-zero: the reference initialises them to 0,
    where a dropped bias would not show), the Blur buffers make_kernel([1, 3, 3, 1])."""
    g = torch.Generator().manual_seed(seed)
    W = {}
    for k, shape in motion_shapes(size).items():
        if k.endswith("kernel"):
            W[PREFIX + k] = blur_kernel()
        else:
            W[PREFIX + k] = ((0.1 if k.endswith("bias") else 1.0) * torch.randn(shape, generator=g)).to(BF16).float()
    return W


def face_frames(T, size, seed=43):
    """uint8 [T, size, size, 3]: smooth seeded gradients plus noise, every byte value possible."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    f = torch.empty(T, size, size, 3)
    for t in range(T):
        for c in range(3):
            a, b, ph = torch.rand(3, generator=g).tolist()
            f[t, :, :, c] = 127.5 + 100 * torch.sin(6.28 * (a * xx + b * yy) / size + 6.28 * ph)
    f += 20 * torch.randn(f.shape, generator=g)
    return f.clamp(0, 255).to(torch.uint8)


# --------------------------------------------------------------------------------------------- the pieces
def preprocess(u8):
    """preprocess_image (diffsynth/utils/__init__.py:60-66) on uint8 [T, H, W, 3] -> planar [T, 3, H, W]."""
    x = u8.permute(0, 3, 1, 2)
    if PURE:
        return x.double() * (2 / 255) + -1
    return x.float().to(BF16) * (2 / 255) + -1


def _cv(x):
    return x.double() if PURE else x.float()


def _out(x):
    return x if PURE else x.to(BF16)


def _w(w, fan_in):
    """`self.weight * self.scale` of the module in its dtype."""
    return (w.double() if PURE else w.to(BF16)) * (1 / math.sqrt(fan_in))


def _b(b):
    return b.double() if PURE else b.to(BF16)


def act(x, bias):
    """fused_leaky_relu, literally: on bf16 tensors each of the three operations rounds."""
    return F.leaky_relu(x + _b(bias).view(1, -1, 1, 1), 0.2) * S2


def conv2d(x, w, stride=1, padding=0):
    cin, k = w.shape[1], w.shape[2]
    return _out(F.conv2d(_cv(x), _cv(_w(w, cin * k * k)), stride=stride, padding=padding))


def blur(x, p0, p1, step=1):
    """upfirdn2d with the [1, 3, 3, 1] kernel and pad (p0, p1), sampled every `step`: float64 sum, one rounding."""
    c = x.shape[1]
    k = blur_kernel().double().view(1, 1, 4, 4).expand(c, 1, 4, 4)
    y = F.conv2d(F.pad(x.double(), [p0, p1, p0, p1]), k, groups=c)
    return _out(y[:, :, ::step, ::step])


def merge(out, skip):
    return (out + skip) / math.sqrt(2)


def res_block(x, W, p):
    o = act(conv2d(x, W[p + "conv1.0.weight"], padding=1), W[p + "conv1.1.bias"])
    o = act(conv2d(blur(o, 2, 2), W[p + "conv2.1.weight"], stride=2), W[p + "conv2.2.bias"])
    s = conv2d(blur(x, 1, 1), W[p + "skip.1.weight"], stride=2)
    return merge(o, s)


def linear(h, w, b):
    return _out(F.linear(_cv(h), _cv(_w(w, w.shape[1]))) + _cv(_b(b) * 1))


def direction_q(w):
    """Direction's Q (custom_qr of weight + 1e-8)."""
    if PURE:
        return torch.linalg.qr(w.double() + 1e-8)[0]
    return torch.linalg.qr((w.to(BF16) + 1e-8).float())[0].to(BF16)


def direction(alpha, q):
    """diag_embed(alpha) @ Q.T summed over dim 1: every product rounded, then a bf16 sum (fp32 inside)."""
    if PURE:
        return alpha @ q.t()
    prod = (alpha.float()[:, None, :] * q.float()[None]).to(BF16)
    return prod.float().sum(-1).to(BF16)


def enc_motion(px, W, p=PREFIX):
    """Encoder.enc_motion on planar px [T, 3, S, S] -> [T, motion_dim]."""
    c = p + "enc.net_app.convs."
    h = act(conv2d(px, W[c + "0.0.weight"]), W[c + "0.1.bias"])
    n = 1
    while c + f"{n}.conv1.0.weight" in W:
        h = res_block(h, W, f"{c}{n}.")
        n += 1
    h = conv2d(h, W[f"{c}{n}.weight"]).flatten(1)
    for i in range(5):
        h = linear(h, W[p + f"enc.fc.{i}.weight"], W[p + f"enc.fc.{i}.bias"])
    return h


def get_motion(px, W, p=PREFIX):
    return direction(enc_motion(px, W, p), direction_q(W[p + "dec.direction.weight"]))


# ------------------------------------------------------------------------------------------- comparisons
def err(got, ref):
    """(rel-L2, max-abs) of got against ref in float64."""
    d = got.double() - ref.double()
    return (d.norm() / ref.double().norm()).item(), d.abs().max().item()


def within_floor(got, ref64, floor_bf16, tag):
    """The floor is the reference's own bf16 run against its float64 run (both in the fixture): rel <= 1.5 frel +
    2e-3 (the project's relative rule) and max-abs <= 2 fmx -- no additive constant, the outputs are ~0.15; the
    factor 2 allows another fp32 summation order in the stacked blocks."""
    frel, fmx = err(floor_bf16, ref64)
    rel, mx = err(got, ref64)
    print(f"{tag}: rel-L2 {rel:.3e} (floor {frel:.3e}), max-abs {mx:.3e} (floor {fmx:.3e})")
    assert rel <= 1.5 * frel + 2e-3, (tag, rel, frel)
    assert mx <= 2 * fmx, (tag, mx, fmx)


def near_midpoint_rel(x64, rel=2.0 ** -20):
    """True where the float64 value lies within `rel` (relative) of a bf16 rounding midpoint."""
    a = x64.abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -126)))
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)
    r = torch.remainder(a / ulp, 1.0)
    return ((r - 0.5).abs() * ulp <= rel * a) & (a > 0)


def same_or_ambiguous(got, x64, tag, max_share=1e-3):
    """got's bits equal bf16(x64) except where x64 is within 2^-20 relative of a rounding midpoint, and the
    excepted elements -- those that differ there -- are at most 0.1 % of all.  (Sums of a few bf16 values lie on a
    coarse grid, so exact ties are common, a percent or so of a normal input; a tie rounds to even in any exact
    arithmetic and needs no exception.  Only an inexact fp32 sum next to a midpoint does.)"""
    got, x64 = got.cpu().contiguous(), x64.contiguous()
    if got.numel() == 0:
        return
    want = x64.to(BF16)
    diff = got.view(torch.int16) != want.view(torch.int16)
    diff &= ~((got.float() == 0) & (want.float() == 0))                # -0 == +0
    amb = near_midpoint_rel(x64)
    print(f"{tag}: {int(diff.sum())} of {diff.numel()} differ, {int((diff & ~amb).sum())} of them outside the "
          f"midpoint window ({int(amb.sum())} elements inside it)")
    assert not bool((diff & ~amb).any()), tag
    assert int(diff.sum()) <= max_share * diff.numel(), (tag, int(diff.sum()), diff.numel())


def blur_ref64(x, bias_act, p0, p1, step):
    """vs_lrelu_blur's contract in float64 on channels-last x [n, H, W, C] (already activated when bias_act is
    given as the activated tensor): the exact sum, not rounded."""
    a = (x if bias_act is None else bias_act).double().permute(0, 3, 1, 2)
    c = a.shape[1]
    k = blur_kernel().double().view(1, 1, 4, 4).expand(c, 1, 4, 4)
    y = F.conv2d(F.pad(a, [p0, p1, p0, p1]), k, groups=c)[:, :, ::step, ::step]
    return y.permute(0, 2, 3, 1).contiguous()


def all_finite_bf16():
    b = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)
    return b[torch.isfinite(b.float())]
