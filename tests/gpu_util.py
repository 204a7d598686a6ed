import math

import torch

BF16 = torch.bfloat16


def to_dev(t):
    return t.to("cuda")


def err(a, b):
    """(max abs error, relative L2 error) of a bf16 result vs a reference."""
    a, b = a.float().cpu(), b.float().cpu()
    d = (a - b)
    return d.abs().max().item(), (d.norm() / (b.norm() + 1e-30)).item()


# ---------------------------------------------------------------------------------------------------
# Helpers of the direct kernel-parity tier (test_t5_kernels_gpu, test_batched_gemm_gpu,
# test_vae_helpers_gpu, test_elementwise_edges_gpu, the row-kernel edge tests of test_kernels_gpu).
# Everything below runs on CPU tensors too: tests/test_kernel_refs_cpu.py checks the references'
# own preconditions without a GPU.
# ---------------------------------------------------------------------------------------------------
SENT_BF16 = 0x7FC0          # a quiet NaN: the pre-fill of every output buffer and of unread input pads
SENT_F32 = 0x7FC00000


def ceil32(n):
    return (n + 31) // 32 * 32


def bits(t):
    """The raw bit pattern of a bf16 / fp32 / uint8 tensor as an integer tensor (same shape)."""
    if t.dtype == BF16:
        return t.view(torch.int16)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t


def sentinel(shape, dtype=BF16, device="cuda"):
    """A tensor filled with the NaN sentinel bit pattern."""
    if isinstance(shape, int):
        shape = (shape,)
    if dtype == BF16:
        return torch.full(shape, SENT_BF16, dtype=torch.int16, device=device).view(BF16)
    if dtype == torch.float32:
        return torch.full(shape, SENT_F32, dtype=torch.int32, device=device).view(torch.float32)
    raise ValueError(dtype)


def untouched(t):
    """Every element of t still holds the sentinel bit pattern."""
    pat = SENT_BF16 if t.dtype == BF16 else SENT_F32
    return bool((bits(t) == pat).all())


def bit_zero(t):
    """Every element of t is +0 (all bits clear)."""
    return bool((bits(t) == 0).all())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.cpu()), bits(b.cpu()))


def same_bits_or_nan(a, b):
    """Elementwise: identical bit patterns, or NaN on both sides (NaN compares as NaN)."""
    a, b = a.cpu(), b.cpu()
    return (bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))


def bf16_ord(t):
    """bf16 -> int32 whose differences count bf16 ulps (monotone in the value; +0 and -0 both 0)."""
    i = t.cpu().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = i & 0x7FFF
    return torch.where(i >= 0x8000, -mag, mag)


def call(name, *args):
    """One C-ABI entry through vstyler._lib (argument types from its signature table), checked."""
    from vstyler import _lib
    _lib.check(getattr(_lib.load(), name)(*args))


def call_rc(name, *args):
    """The same, returning the VS_* code instead of raising."""
    from vstyler import _lib
    return getattr(_lib.load(), name)(*args)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------ softmax references
SOFTMAX_REL = 2.0 ** -8     # one bf16 ulp: half an ulp of rounding + the fp32 expf / division error


def softmax_within(got, ref64):
    """|got - ref64| <= 2^-8 ref64 + 1e-30 per element (got bf16, ref64 float64)."""
    d = (got.cpu().double() - ref64).abs()
    return d <= SOFTMAX_REL * ref64 + 1e-30


def t5_softmax_ref(s, emb, buckets, keymask, head0, nz):
    """The oracle's expression (oracle/t5_oracle.py t5_attention): bf16(s) + bf16 bias with finfo.min on
    masked keys, added as a bf16 tensor op, softmax in float64.  s fp32 [nz, L, L]; emb bf16
    [buckets, nheads]; buckets int [L, L]; keymask int [L].  Returns (v bf16 [nz, L, L], softmax f64)."""
    L = s.shape[-1]
    pos_bias = emb[buckets.long()].permute(2, 0, 1)[head0:head0 + nz]
    attn_bias = torch.zeros(nz, L, L, dtype=BF16)
    attn_bias += pos_bias
    attn_bias.masked_fill_(keymask.view(1, 1, L) == 0, torch.finfo(BF16).min)
    v = (s.to(BF16).float() + attn_bias.float()).to(BF16)
    return v, torch.softmax(v.double(), dim=-1)


# ------------------------------------------------------------------------ rounding-midpoint ambiguity
def near_bf16_midpoint(x64, ulps32):
    """True where the float64 value lies within `ulps32` fp32 ulps of a bf16 rounding midpoint (a value
    whose fp32 pattern ends in 0x8000): a last-place difference of an fp32 evaluation can round it to
    either bf16 neighbour."""
    a = x64.abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -126)))
    u = a / torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23)     # in fp32 ulps, [2^23, 2^24)
    r = torch.remainder(u, 65536.0)
    return ((r - 32768.0).abs() <= ulps32) & (a > 0) & torch.isfinite(a)


def t5_gelu_inputs():
    """g: every bf16 bit pattern + 37 seeded extras (n % 256 != 0); a: seeded N(0, 1)."""
    gen = torch.Generator().manual_seed(1234)
    allbits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)
    g = torch.cat([allbits, (3.0 * torch.randn(37, generator=gen)).to(BF16)])
    a = torch.randn(g.numel(), generator=gen).to(BF16)
    return a, g


def t5_gelu_mul_ref(a, g):
    """(ref, ambiguous): ref = bf16(a * gelu_bf16(g)) (oracle/t5_oracle.py gelu_bf16); ambiguous marks
    the elements whose tanh, evaluated in float64, lies within 4 fp32 ulps of a bf16 rounding midpoint
    -- the one step of the chain a device tanhf may round the other way.  From the reference alone."""
    from oracle import t5_oracle as T
    ref = (a.float() * T.gelu_bf16(g).float()).to(BF16)
    f = lambda t: t.float()  # noqa: E731
    x3 = (f(g) * f(g) * f(g)).to(BF16)
    t = (0.044715 * f(x3)).to(BF16)
    t = (f(g) + f(t)).to(BF16)
    t = (math.sqrt(2.0 / math.pi) * f(t)).to(BF16)
    amb = near_bf16_midpoint(torch.tanh(t.double()), 4)
    return ref, amb


def sinusoid_inputs():
    """Every integer timestep 0..1000 and 50 seeded fractional ones, as bf16."""
    gen = torch.Generator().manual_seed(77)
    frac = 1000.0 * torch.rand(50, generator=gen)
    return torch.cat([torch.arange(1001, dtype=torch.float32), frac]).to(BF16)


def sinusoid_ref(dim, t):
    """(ref, ambiguous): oracle sinusoidal_embedding_1d and the elements whose float64 cos / sin lies
    within 4 fp64 ulps of a point where the conversion to bf16 (through fp32, as both sides convert)
    changes its result."""
    from oracle import wan_oracle as O
    ref = O.sinusoidal_embedding_1d(dim, t)
    half = dim // 2
    ang = torch.outer(t.double(), torch.pow(10000, -torch.arange(half, dtype=torch.float64).div(half)))
    x = torch.cat([torch.cos(ang), torch.sin(ang)], dim=1)
    lo, hi = x.clone(), x.clone()
    inf = torch.tensor(float("inf"), dtype=torch.float64)
    for _ in range(4):
        lo, hi = torch.nextafter(lo, -inf), torch.nextafter(hi, inf)
    amb = lo.float().to(BF16) != hi.float().to(BF16)           # by value: an exact zero is not ambiguous
    return ref, amb


# --------------------------------------------------------------------------------- row-kernel references
ROW_LN_DIMS = [8, 72, 1024, 1032, 5120, 5128, 8192]
ROW_RMS_DIMS = [128, 1152, 5120, 5248]
ROW_BOUND = 2.0 ** -7       # one bf16 ulp (relative upper bound) per rounding an fp32-level change can flip
ROW_MIN_IDENTICAL = 0.99


def row_inputs(rows, dim, seed):
    """x bf16 [rows, dim] (N(0, 4) + a per-row offset), shift / scale bf16 [rows, dim] (one pair per row:
    rows_per_batch = 1), affine weight / bias bf16 [dim]."""
    g = torch.Generator().manual_seed(seed * 100003 + dim)
    x = (2.0 * torch.randn(rows, dim, generator=g) + torch.randn(rows, 1, generator=g)).to(BF16)
    mod = (0.3 * torch.randn(rows, 2, dim, generator=g)).to(BF16)
    w = (1 + 0.1 * torch.randn(dim, generator=g)).to(BF16)
    b = (0.1 * torch.randn(dim, generator=g)).to(BF16)
    return x, mod, w, b


def _ln_normalised(x, eps, dtype):
    xf = x.to(dtype)
    mean = xf.mean(dim=-1, keepdim=True)
    var = (xf - mean).pow(2).mean(dim=-1, keepdim=True)
    return (xf - mean) * torch.rsqrt(var + eps)


def ln_modulate_ref(x, shift, scale, eps=1e-6, dtype=torch.float64):
    """LayerNorm -> bf16 -> modulate with the oracle's rounding points (wan_oracle layer_norm + modulate),
    the statistics in `dtype`.  Returns (ref bf16, bound): bound = 2^-7 (|n (1 + scale)| + |ref|)."""
    n = _ln_normalised(x, eps, dtype)
    nb = n.float().to(BF16)
    s1 = (1 + scale.float()).to(BF16)
    ref = ((nb.float() * s1.float()).to(BF16).float() + shift.float()).to(BF16)
    bound = ROW_BOUND * ((n.double() * s1.double()).abs() + ref.double().abs())
    return ref, bound


def ln_affine_ref(x, w, b, eps=1e-6, dtype=torch.float64):
    """LayerNorm with affine weight / bias -> bf16 (one rounding).  bound = 2^-7 |ref| (one bf16 ulp at
    that rounding) + 2^-20 (|n w| + |b|) (sixteen fp32 ulps of the terms: the fp32 statistics and the
    multiply-add before the rounding, which matter only where n w + b cancels)."""
    n = _ln_normalised(x, eps, dtype)
    y = n.double() * w.double() + b.double()
    ref = y.float().to(BF16)
    bound = ROW_BOUND * ref.double().abs() + 2.0 ** -20 * ((n.double() * w.double()).abs() + b.double().abs())
    return ref, bound


def rms_rope_ref(x, w, eps=1e-6, freqs=None, heads=1, dtype=torch.float64):
    """RMSNorm (wan_oracle.rms_norm's rounding points, the mean square in `dtype`) and, with freqs
    (complex128 [rows, 1, 64]), the interleaved RoPE in complex128 (wan_oracle.rope_apply).
    bound: without RoPE 2^-7 (|x r w| + |ref|) -- one ulp where bf16(x r) flips, carried through w, and
    one at the output rounding; with RoPE the two upstream roundings each move a rotated term by one
    ulp, 2^-6 (|a cos| + |b sin|) over the pair (a, b), plus 2^-7 |ref| at the output rounding."""
    xf = x.to(dtype)
    r = torch.rsqrt(xf.pow(2).mean(dim=-1, keepdim=True) + eps)
    n = (xf * r).float().to(BF16)
    y = (n.float() * w.float()).to(BF16)
    mag = (xf * r).double().abs() * w.double().abs()
    if freqs is None:
        return y, ROW_BOUND * (mag + y.double().abs())
    rows, dim = x.shape
    yc = torch.view_as_complex(y.double().reshape(rows, heads, -1, 2))
    ref = torch.view_as_real(yc * freqs).flatten(1).float().to(BF16)
    m2 = mag.reshape(rows, heads, -1, 2)
    c, s = freqs.real.abs(), freqs.imag.abs()
    re = m2[..., 0] * c + m2[..., 1] * s
    im = m2[..., 0] * s + m2[..., 1] * c
    rot = torch.stack([re, im], dim=-1).reshape(rows, dim)
    return ref, 2 * ROW_BOUND * rot + ROW_BOUND * ref.double().abs()


class RowTally:
    """The row kernels' bar: every element within its bound of the float64-statistics reference
    (asserted per call of check) and >= 99 % of the elements of one test case (all its row counts and
    stride forms pooled: a dim-8 row alone has too few elements to express 99 %) bit-identical."""

    def __init__(self, what):
        self.what, self.same, self.total = what, 0, 0

    def check(self, got, ref, bound, what=""):
        got, ref = got.cpu(), ref.cpu()
        d = (got.double() - ref.double()).abs()
        self.same += int((bits(got) == bits(ref)).sum())
        self.total += got.numel()
        worst = (d - bound).max().item()
        assert torch.isfinite(got.float()).all(), (self.what, what)
        assert bool((d <= bound).all()), (self.what, what, worst)

    def finish(self):
        share = self.same / max(self.total, 1)
        print(f"{self.what}: bit-identical share {share:.5f} of {self.total}")
        assert share >= ROW_MIN_IDENTICAL, (self.what, share)
        return share
