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


# ------------------------------------------------------------------------------ attention references
# The contract of vs_attn_fwd (both kernels, every route): Q pre-scaled by c = fp32(scale) * fp32(log2 e)
# with ONE bf16 rounding, p = exp2(S [- m]) rounded to bf16, fp32 accumulation of P V and of l = sum p,
# store bf16(acc * (1 / l)).  Two references restate it in float64 (test_attention_exact_gpu.py, the
# preconditions of both in test_kernel_refs_cpu.py):
#   * attn_exact_inputs: inputs on which every step but the last is exact in fp32, so the answer is
#     known to the bit wherever the float64 ratio is not next to a bf16 rounding midpoint;
#   * attn_random_*: random inputs with a per-element bound derived from the two bf16 roundings.
ATTN_HD = 128
ATTN_EXACT_SCALE = torch.tensor(math.log(2.0), dtype=torch.float32).item()      # float32(ln 2)
ATTN_WINDOW = 8             # fp32 ulps around a bf16 midpoint: device 1/l, the product, a 1-ulp exp2 in l ~ 3.5
ATTN_MAX_AMBIGUOUS = 0.01   # a condition on the INPUTS (asserted from the reference alone), no tolerance
ATTN_BOUND = 2.0 ** -8      # |got - o| <= 2^-8 (|o| + A): see attn_within
ATTN_ROUTES = {"default": {}, "impl8": {"attn_impl": 8}, "nc0": {"attn_nc": 0}, "mfma32": {"attn_mfma": 32}}
W4_LMIN = 2.0 ** -4         # csrc/attention.h: attn_fwd_w4 sends an item with a row sum below it to the redo


def attn_prescale(q, scale):
    """bf16(fp32(q) * c), c = fp32(scale) * 1.4426950408889634f: the kernels' own product and rounding."""
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    return (q.float() * c.to(q.device)).to(BF16)


def attn_exact_inputs(B, Sq, Skv, H, seed, shared_kv=False, r_rows=None):
    """q [B*Sq, H*128], k, v [(1 if shared_kv else B)*Skv, H*128] (bf16, CPU) of the exact problem:
    q: per (row, head) a 1 at a seeded column 0..126 and a seeded integer r in -2..2 at column 127 (a
       per-row shift that cancels in the ratio); r_rows {row: r} overrides r for that row of every
       (sample, head);
    k: columns 0..126 seeded integers -lev, lev 0..3; column 127 = 1  -> every score is an integer;
    v: zero except where (key + column + 3 head) % 8 == 0, there seeded integers 1..4."""
    g = torch.Generator().manual_seed(seed)
    Bk = 1 if shared_kv else B
    col = torch.randint(0, 127, (B * Sq, H), generator=g)
    r = torch.randint(-2, 3, (B * Sq, H), generator=g)
    for row, val in (r_rows or {}).items():
        r.view(B, Sq, H)[:, row, :] = val
    q = torch.zeros(B * Sq, H, ATTN_HD)
    q.scatter_(2, col.unsqueeze(-1), 1.0)
    q[:, :, 127] = r.float()
    k = -torch.randint(0, 4, (Bk * Skv, H, ATTN_HD), generator=g).float()
    k[:, :, 127] = 1.0
    val = torch.randint(1, 5, (Bk * Skv, H, ATTN_HD), generator=g).float()
    j = torch.arange(Skv).repeat(Bk).view(-1, 1, 1)
    h = torch.arange(H).view(1, -1, 1)
    d = torch.arange(ATTN_HD).view(1, 1, -1)
    v = torch.where((j + d + 3 * h) % 8 == 0, val, torch.zeros(()))
    flat = lambda t: t.reshape(t.shape[0], H * ATTN_HD).to(BF16)  # noqa: E731
    return flat(q), flat(k), flat(v)


def attn_ref64(q, k, v, H, B, scale, shared_kv=False, exact=False):
    """The contract in float64 on the tensors' device, chunked over query rows.  q [B*Sq, >= H*128] rows,
    k / v [B*Skv or Skv, ...] (views allowed).  Returns a dict: o = sum p v / l and A = sum p |v| / l
    ([B*Sq, H*128]), l = sum exp2(S) and smin / smax, the extreme scores ([B*Sq, H]), from
    S = bf16(q c) . k.  exact=True also checks the exact problem's preconditions (the pre-scaling leaves
    q unchanged; integer scores; every P V and l partial sum, attn_fwd_w4's up to 63 padded keys of
    weight 1 included, a multiple of the row's smallest p below 2^24 of them) and returns them in `pre`."""
    dev = q.device
    Sq, Skv = q.shape[0] // B, k.shape[0] // (1 if shared_kv else B)
    D = H * ATTN_HD
    qs = attn_prescale(q[:, :D], scale)
    pre = {"q_unchanged": same_bits(qs, q[:, :D].contiguous()), "integer": True, "exact": True, "pv_max": 0.0}
    out = {n: torch.empty(B * Sq, D, dtype=torch.float64, device=dev) for n in ("o", "A")}
    out.update({n: torch.empty(B * Sq, H, dtype=torch.float64, device=dev) for n in ("l", "smin", "smax")})
    step = max(1, (1 << 22) // Skv)
    for b in range(B):
        kb = 0 if shared_kv else b
        for h in range(H):
            cs = slice(h * ATTN_HD, (h + 1) * ATTN_HD)
            k64 = k[kb * Skv:(kb + 1) * Skv, cs].double()
            v64 = v[kb * Skv:(kb + 1) * Skv, cs].double()
            for r0 in range(b * Sq, (b + 1) * Sq, step):
                rs = slice(r0, min(r0 + step, (b + 1) * Sq))
                s = qs[rs, cs].double() @ k64.t()
                m = s.max(dim=1, keepdim=True).values
                p = torch.exp2(s - m)
                lr = p.sum(dim=1, keepdim=True)
                out["o"][rs, cs] = (p @ v64) / lr
                pav = p @ v64.abs()
                out["A"][rs, cs] = pav / lr
                out["l"][rs, h] = (lr * torch.exp2(m)).squeeze(1)
                out["smax"][rs, h] = m.squeeze(1)
                smin = s.min(dim=1, keepdim=True).values
                out["smin"][rs, h] = smin.squeeze(1)
                if exact:
                    pre["integer"] = pre["integer"] and bool((s == s.round()).all())
                    # in units of the row's smallest p (every partial sum is a whole number of them)
                    units = (pav.max(dim=1, keepdim=True).values * torch.exp2(m) + 64.0) * torch.exp2(-smin)
                    pre["exact"] = pre["exact"] and bool((units < 2.0 ** 24).all())
                    pre["pv_max"] = max(pre["pv_max"], (pav * torch.exp2(m)).max().item())
    out["pre"] = pre
    return out


def attn_exact_ref(q, k, v, H, B, shared_kv=False, window=ATTN_WINDOW):
    """(ref bf16, ambiguous bool, ref64 dict) of the exact problem at scale float32(ln 2): float64 ->
    fp32 -> bf16, and the elements within `window` fp32 ulps of a bf16 rounding midpoint."""
    r = attn_ref64(q, k, v, H, B, ATTN_EXACT_SCALE, shared_kv, exact=True)
    return r["o"].float().to(BF16), near_bf16_midpoint(r["o"], window), r


def attn_exact_preconditions(r, amb, smin=-5, smax=2):
    """The exact problem's preconditions on a reference (r, amb) of attn_exact_ref; returns the ambiguous
    share.  Rows with an overridden r (the redo-threshold case) widen the score range: pass it."""
    pre = r["pre"]
    assert pre["q_unchanged"], "bf16(q * c) != q at scale float32(ln 2)"
    assert pre["integer"] and pre["exact"], pre
    assert pre["pv_max"] < 2.0 ** 19, pre
    assert r["smin"].min().item() >= smin and r["smax"].max().item() <= smax, (r["smin"].min(), r["smax"].max())
    share = amb.double().mean().item()
    assert share <= ATTN_MAX_AMBIGUOUS, share
    return share


def attn_exact_verdict(got, ref, amb, ref64):
    """The exact bar on one result (got bf16 [rows, H*128]): every element within one bf16 ulp of ref,
    every non-ambiguous element bit-identical, exact zeros +0.  Returns (ok, text)."""
    got, ref, amb = got.cpu(), ref.cpu(), amb.cpu()
    d = (bf16_ord(got) - bf16_ord(ref)).abs()
    finite = bool(torch.isfinite(got.float()).all())
    diff = bits(got) != bits(ref)
    hard = diff & ~amb
    zeros = ref64.cpu() == 0
    zero_ok = bool((bits(got)[zeros] == 0).all())
    text = (f"max ulp {int(d.max())}, differing {int(diff.sum())} ({int(hard.sum())} not ambiguous) of {got.numel()}, "
            f"ambiguous {int(amb.sum())}, exact zeros {int(zeros.sum())} (+0: {zero_ok}), finite {finite}")
    return finite and int(d.max()) <= 1 and not bool(hard.any()) and zero_ok, text


def attn_midpoint_distance(got, ref, ref64):
    """For the elements where got != ref by one bf16 ulp: the distance of the float64 value from the
    bf16 rounding midpoint, in fp32 ulps (the measurement behind ATTN_WINDOW); empty when none differ."""
    got, ref, x = got.cpu(), ref.cpu(), ref64.cpu()
    sel = bits(got) != bits(ref)
    a = x[sel].abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** -126)))
    u = a / torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23)
    return (torch.remainder(u, 65536.0) - 32768.0).abs()


def attn_add_ref(o0, ref, amb, ref64):
    """vs_attn_fwd_add's o = bf16(o0 + bf16(attention)) from the exact reference: (want, other).  The fp32
    sum of an integer o0 in -4..4 and a bf16 value is exact (asserted), so the second rounding has one
    answer; an ambiguous first rounding may land on ref's bf16 neighbour across the midpoint, whose sum
    is `other` (= want where not ambiguous): a result must equal want or other."""
    def add(x):
        s32 = o0.float() + x.float()
        assert torch.equal(s32.double(), o0.double() + x.double())
        return s32.to(BF16)
    o = bf16_ord(ref) + torch.where(ref64 > ref.double(), 1, -1)
    mag = o.abs()
    pat = torch.where(o < 0, mag | 0x8000, mag)
    across = (pat - ((pat & 0x8000) << 1)).to(torch.int16).view(BF16)
    want = add(ref)
    return want, torch.where(amb, add(across), want)


def attn_random_inputs(B, Sq, Skv, H, seed):
    """q ~ 2 N(0, 1), k, v ~ N(0, 1) as bf16 [B*S, H*128] (CPU)."""
    g = torch.Generator().manual_seed(seed)
    D = H * ATTN_HD
    return ((2.0 * torch.randn(B * Sq, D, generator=g)).to(BF16), torch.randn(B * Skv, D, generator=g).to(BF16),
            torch.randn(B * Skv, D, generator=g).to(BF16))


def attn_spike_inputs(kind):
    """The inputs of test_kernels_gpu's test_attention_online_rescale_spike / _overflow_spike /
    _first_tile_low_scores[late] / _rescale_many, rebuilt: (q, k, v, H, B) as [B*S, H*128] rows."""
    def rnd(*shape, seed):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(BF16)
    if kind == "rescale_spike":
        S, H = 512, 1
        q, k, v = rnd(S, 128, seed=30), rnd(S, 128, seed=31), rnd(S, 128, seed=32)
        q[5] = 4.0
        k[400] = 4.0
    elif kind == "overflow_spike":
        S, H = 512, 1
        q, k, v = rnd(S, 128, seed=33), rnd(S, 128, seed=34), rnd(S, 128, seed=35)
        for row, key in ((3, 10), (5, 300), (9, 360), (200, 511)):
            q[row] = 6.0
            k[key] = 6.0
    elif kind in ("low_scores", "low_scores_late"):
        S, H = 512, 1
        g = torch.Generator().manual_seed(36)
        u = torch.ones(128)
        k = (0.1 * torch.randn(1, S, 128, generator=g) + u).to(BF16)[0]
        if kind == "low_scores_late":
            k[64:] = torch.randn(S - 64, 128, generator=g).to(BF16)
        q = torch.randn(1, S, 128, generator=g).to(BF16)[0]
        for row in (0, 7, 200, 511):
            q[row] = (-4.0 * u + 0.01 * torch.randn(128, generator=g)).to(BF16)
        v = torch.randn(1, S, 128, generator=g).to(BF16)[0]
    elif kind == "rescale_many":
        S, H = 2048, 2
        q, k, v = rnd(1, S, 256, seed=50)[0], rnd(1, S, 256, seed=51)[0], rnd(1, S, 256, seed=52)[0]
        for key, row, a in ((300, 7, 0.3), (900, 7, 0.5), (1500, 7, 0.8), (130, 40, 0.4), (1999, 300, 0.6),
                            (64, 1000, 0.35), (1000, 2047, 0.7), (2047, 12, 0.9)):
            k[key] = (q[row].float() * a).to(BF16)
    else:
        raise ValueError(kind)
    return q, k, v, H, 1


def attn_within(got, r):
    """error / bound per element, bound = 2^-8 (|o| + A) from attn_ref64's dict: half a bf16 ulp on each
    p moves the numerator by 2^-9 A and the denominator by 2^-9 |o| (relative 2^-9 of l, times o), the
    output rounding is 2^-9 |o|, and the A term carries about twice the remaining slack for the fp32 sums."""
    err_ = (got.double().to(r["o"].device) - r["o"]).abs()
    bound = ATTN_BOUND * (r["o"].abs() + r["A"])
    return err_ / torch.clamp(bound, min=1e-300)


# The GPU cases of test_attention_exact_gpu.py, by name: the arguments of attn_exact_inputs.  One table,
# so that test_kernel_refs_cpu.py checks the preconditions of exactly the inputs the GPU tests use.
ATTN_EDGE_SKV_W8 = [1, 7, 31, 32, 33, 63, 64, 65, 129, 192]                       # < 4 key tiles: 8-wave on every route
ATTN_EDGE_SKV_W4 = [193, 224, 225, 255, 256, 257, 288, 289, 319, 320, 321, 383, 384, 385, 448, 449]   # nkv 4..8
ATTN_EDGE_SQ = [1, 63, 64, 65, 255, 256, 257]
ATTN_REDO_ROWS = {17: -10, 290: -11}      # q-block 0 keeps l >= 2^-4 (stays on attn_fwd_w4), q-block 1 falls below


def attn_exact_cases():
    c = {}
    for skv in ATTN_EDGE_SKV_W8 + ATTN_EDGE_SKV_W4:
        c[f"edge_skv{skv}"] = dict(B=2, Sq=300, Skv=skv, H=2, seed=1000 + skv)
    for sq in ATTN_EDGE_SQ:
        c[f"edge_sq{sq}"] = dict(B=2, Sq=sq, Skv=257, H=2, seed=2000 + sq)
    c["fused_qkv"] = dict(B=2, Sq=321, Skv=321, H=2, seed=3001)
    c["shared_kv"] = dict(B=2, Sq=300, Skv=257, H=2, seed=3002, shared_kv=True)
    c["redo"] = dict(B=2, Sq=300, Skv=193, H=2, seed=3003, r_rows=ATTN_REDO_ROWS)
    c["switch"] = dict(B=2, Sq=9000, Skv=520, H=4, seed=3004)
    c["split"] = dict(B=1, Sq=23040, Skv=2079, H=3, seed=3005)
    c["add_skv257"] = dict(B=2, Sq=300, Skv=257, H=2, seed=3006)
    c["add_skv449"] = dict(B=2, Sq=300, Skv=449, H=2, seed=3007)
    return c


ATTN_RANDOM_SHAPES = [(2, 300, 77, 2), (2, 300, 300, 2), (2, 300, 449, 2), (1, 1000, 2048, 2)]
ATTN_SPIKE_KINDS = ["rescale_spike", "overflow_spike", "low_scores", "low_scores_late", "rescale_many"]
ATTN_BOUND_CASES = ["x".join(map(str, s)) for s in ATTN_RANDOM_SHAPES] + ATTN_SPIKE_KINDS


def attn_bound_case(name):
    """(q, k, v, H, B) of a bound-tier case: "BxSqxSkvxH" random inputs or a spike kind."""
    if name in ATTN_SPIKE_KINDS:
        return attn_spike_inputs(name)
    B, Sq, Skv, H = (int(x) for x in name.split("x"))
    return (*attn_random_inputs(B, Sq, Skv, H, seed=5000 + Skv), H, B)


def attn_add_o0(shape, skv):
    """vs_attn_fwd_add's prior output: seeded integers in -4..4 (bf16, CPU)."""
    return torch.randint(-4, 5, tuple(shape), generator=torch.Generator().manual_seed(4000 + skv)).to(BF16)


def attn_emulate_fp32(q, k, v, H, B, scale, shared_kv=False, drop_last_key=False, l_add=0.0, truncate_p=False):
    """The contract evaluated in fp32 on the CPU (optimistic form: p = exp2(S) without a reference max,
    so for moderate scores only): what a correct kernel computes, for test_kernel_refs_cpu.py to hold
    the references' bars against -- and, with one of the three arithmetic mutations, what a subtly wrong
    one does."""
    Sq, Skv = q.shape[0] // B, k.shape[0] // (1 if shared_kv else B)
    qs = attn_prescale(q, scale).float()
    out = torch.empty(B * Sq, H * ATTN_HD, dtype=BF16)
    n = Skv - 1 if drop_last_key else Skv
    for b in range(B):
        kb = 0 if shared_kv else b
        for h in range(H):
            cs = slice(h * ATTN_HD, (h + 1) * ATTN_HD)
            rs = slice(b * Sq, (b + 1) * Sq)
            p = torch.exp2(qs[rs, cs] @ k[kb * Skv:kb * Skv + n, cs].float().t())
            if truncate_p:
                p = (p.view(torch.int32) & -65536).view(torch.float32)
            p = p.to(BF16).float()
            lsum = p.sum(dim=1, keepdim=True) + l_add
            out[rs, cs] = ((p @ v[kb * Skv:kb * Skv + n, cs].float()) * (1.0 / lsum)).to(BF16)
    return out


# ------------------------------------------------------------------------- VAE conv: the exact problem
# vs_vae_conv in convolution mode (test_vae_conv_exact_gpu.py; preconditions in test_kernel_refs_cpu.py).
# x and w in {-1, 0, 1}, bias an integer in -3..3, the residual an integer in -8..8: every fp32 partial
# sum is an integer far below 2^24, so any summation order gives the same value, and bf16(acc + bias)
# and bf16(that + res) are exact while both stay within +-256 (asserted from the float64 reference).
CONV_EXACT_LIMIT = 256.0
CONV_MIN_NONZERO = 0.5


def conv_density(cin):
    """The share of non-zero entries of x and of w by input width (keeps 27-tap sums within +-256)."""
    return 1.0 if cin <= 32 else 0.5 if cin <= 96 else 0.35 if cin <= 192 else 0.25


def _k3(cin, cout, hw, t, t_lo, res, **kw):
    return dict(cin=cin, cout=cout, k=(3, 3, 3), pad=(2, 1, 1), t=t, hw=hw, out=(t, *hw), t_lo=t_lo, res=res, **kw)


def conv_exact_cases():
    """name -> geometry.  t / hw: the input's frames and source size; out: (t_out, h_out, w_out); y_t: frames
    of y the call may address (default t_out; the buffer gets one guard frame more); keep: frames of y the
    call must not write.  Defaults: n = 2, stride 1, no pad, no up2, t_lo = 0, t_mul = 1, t_add = 0, split = 0,
    with bias, without residual."""
    c = {}
    # k3 causal convs: the launcher each reaches with vae_halo = 1 / 0 is listed in
    # test_vae_conv_exact_gpu.py's docstring
    c["k3_32_96_17x33_t4_res"] = _k3(32, 96, (17, 33), 4, 0, True)
    c["k3_32_96_1x1_t1"] = _k3(32, 96, (1, 1), 1, 0, False)
    c["k3_96_192_16x32_t4_lo1"] = _k3(96, 192, (16, 32), 4, 1, False)
    c["k3_96_192_15x31_t4_lo2_res"] = _k3(96, 192, (15, 31), 4, 2, True)
    c["k3_384_96_16x32_t1_res"] = _k3(384, 96, (16, 32), 1, 0, True)
    c["k3_32_16_17x33_t4_lo1_res"] = _k3(32, 16, (17, 33), 4, 1, True)
    c["k3_32_16_15x31_t1"] = _k3(32, 16, (15, 31), 1, 0, False)
    c["k3_32_3_17x33_t4_lo2"] = _k3(32, 3, (17, 33), 4, 2, False)
    c["k3_32_3_1x1_t4_res"] = _k3(32, 3, (1, 1), 4, 0, True)
    c["k3_32_3_16x32_t1"] = _k3(32, 3, (16, 32), 1, 0, False)
    c["k3_96_64_17x33_t4_lo1_res"] = _k3(96, 64, (17, 33), 4, 1, True)
    c["k3_96_64_16x32_t1"] = _k3(96, 64, (16, 32), 1, 0, False)
    c["k3_64_128_15x31_t4"] = _k3(64, 128, (15, 31), 4, 0, False)
    c["k3_64_128_1x1_t1_res"] = _k3(64, 128, (1, 1), 1, 0, True)
    c["k3_96_100_17x33_t4_lo2_res"] = _k3(96, 100, (17, 33), 4, 2, True)
    c["k3_96_100_16x32_t1"] = _k3(96, 100, (16, 32), 1, 0, False)
    # the same conv writing frames 1.. of a y whose frame 0 must stay (t_add in both epilogues of the halo kernel)
    c["k3_32_96_17x33_t2_tadd"] = _k3(32, 96, (17, 33), 2, 0, True, t_add=1, y_t=3, keep=(0,))
    c["k3_32_16_17x33_t2_tadd"] = _k3(32, 16, (17, 33), 2, 0, False, t_add=1, y_t=3, keep=(0,))
    # Resample upsample2d / 3d: kt = 1 3x3 through the fused nearest-x2 upsample, odd source sizes, 18 x 34
    # ragged against the halo kernel's 16 x 32 tile
    c["up2_96_96"] = dict(cin=96, cout=96, k=(1, 3, 3), pad=(0, 1, 1), t=2, hw=(9, 17), out=(2, 18, 34), up2=True, res=True)
    c["up2_64_64"] = dict(cin=64, cout=64, k=(1, 3, 3), pad=(0, 1, 1), t=2, hw=(9, 17), out=(2, 18, 34), up2=True)
    # Resample downsample: ZeroPad2d((0, 1, 0, 1)) + 3x3 stride 2 (only the even size reads the zero row / column)
    for h, w in ((8, 12), (7, 11)):
        c[f"down_{h}x{w}"] = dict(cin=64, cout=64, k=(1, 3, 3), stride=(1, 2, 2), t=2, hw=(h, w),
                                  out=(2, (h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1))
    # downsample3d's time conv: stride 2 over frames (2j, 2j + 1, 2j + 2) into frames 1.. of y
    for t in (3, 4, 5):
        to = (t - 1) // 2
        c[f"time_down_t{t}"] = dict(cin=64, cout=64, k=(3, 1, 1), stride=(2, 1, 1), t=t, hw=(5, 7), out=(to, 5, 7),
                                    t_add=1, y_t=1 + to, keep=(0,))
    # upsample3d's time conv: frames 1.. only (t_lo = 1), channel halves interleaved into frames 2j + 1, 2j + 2
    for ch in (32, 64):
        for t in (2, 3):
            c[f"time_up_c{ch}_t{t}"] = dict(cin=ch, cout=2 * ch, k=(3, 1, 1), pad=(1, 0, 0), t=t, hw=(5, 7),
                                            out=(t - 1, 5, 7), t_lo=1, t_mul=2, t_add=1, split=ch, y_t=1 + 2 * (t - 1),
                                            keep=(0,))
    # AttentionBlock's proj: 1x1x1 with the residual, into a given y
    c["proj_96"] = dict(cin=96, cout=96, k=(1, 1, 1), t=2, hw=(6, 10), out=(2, 6, 10), res=True)
    # the load pipeline: nsteps = cin / 32 = 1..7 K-steps (every residue of the three-stage rotation and the
    # nsteps > 1 / > 2 prologue branches), M = 2 * 10 * 15 = 300 pixels (a ragged 256-pixel tile)
    for s in range(1, 8):
        c[f"steps{s}"] = dict(cin=32 * s, cout=96, k=(1, 1, 1), t=1, hw=(10, 15), out=(1, 10, 15), res=s % 2 == 0)
    return c


CONV_STEP_CASES = [f"steps{s}" for s in range(1, 8)]
CONV_PIPELINES = [(pxb, pre) for pxb in (1, 2) for pre in (1, 2, 3)]


def conv_halo_eligible(c):
    """csrc/vae.hip halo_nb() restated for the cases above: 0 (the per-tap kernel only), or the NB of
    the patch-resident kernel that vae_halo = 1 selects."""
    ok = (c["k"][1:] == (3, 3) and c.get("stride", (1, 1, 1)) == (1, 1, 1) and c.get("pad", (0, 0, 0))[1:] == (1, 1)
          and c.get("split", 0) == 0)
    return 0 if not ok else 3 if c["cout"] % 96 == 0 else 1 if c["cout"] <= 32 else 0


def conv_ldy(c):
    """cout rounded up to 4 (8 where the halo kernel's NB = 3 epilogue may run) + 8 pad channels."""
    r = 8 if conv_halo_eligible(c) == 3 else 4
    return (c["cout"] + r - 1) // r * r + 8


_CONV_CACHE = {}


def conv_exact_problem(name):
    """The inputs and the float64 answer of one case, computed once per process and never modified (CPU
    tensors): x [n, t, h, w, cin] bf16 with NaN in the frames below t_lo, w [cout, cin, kt, kh, kw] bf16,
    bias bf16 [cout], res (bf16 buffer of y's geometry, NaN outside the written elements, or None), want
    (bf16 buffer of y's geometry [n, y_t + 1, h_out, w_out, ldy]: the exact answer where the call writes,
    the sentinel everywhere else), written (bool, same shape) and pre: the reference's own preconditions."""
    if name in _CONV_CACHE:
        return _CONV_CACHE[name]
    import torch.nn.functional as F
    c = conv_exact_cases()[name]
    n, cin, cout, (kt, kh, kw) = c.get("n", 2), c["cin"], c["cout"], c["k"]
    t, (h, w), (to, ho, wo) = c["t"], c["hw"], c["out"]
    st, pad = c.get("stride", (1, 1, 1)), c.get("pad", (0, 0, 0))
    t_lo, t_mul, t_add, split = c.get("t_lo", 0), c.get("t_mul", 1), c.get("t_add", 0), c.get("split", 0)
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    d = conv_density(cin)

    def tern(shape):
        return torch.randint(-1, 2, shape, generator=g).double() * (torch.rand(shape, generator=g) < d)
    x64 = tern((n, t, h, w, cin))
    w64 = tern((cout, cin, kt, kh, kw))
    bias64 = torch.randint(-3, 4, (cout,), generator=g).double()
    # the reference: X zero outside [t_lo, t_in) x [0, H) x [0, W) of the (upsampled) input, explicitly
    xz = x64.permute(0, 4, 1, 2, 3).clone()
    xz[:, :, :t_lo] = 0
    if c.get("up2"):
        xz = xz.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    back = [max(0, (o - 1) * s + k - 1 - p - (i - 1)) for o, s, k, p, i in zip((to, ho, wo), st, (kt, kh, kw), pad, xz.shape[2:])]
    xz = F.pad(xz, (pad[2], back[2], pad[1], back[1], pad[0], back[0]))
    acc = F.conv3d(xz, w64, None, stride=st)[:, :, :to, :ho, :wo]
    assert acc.shape[2:] == (to, ho, wo)
    r1 = acc + bias64.view(1, -1, 1, 1, 1)
    y_t, ldy = c.get("y_t", to), conv_ldy(c)
    shape = (n, y_t + 1, ho, wo, ldy)
    want = sentinel(shape, device="cpu")
    written = torch.zeros(shape, dtype=torch.bool)
    res = sentinel(shape, device="cpu") if c.get("res") else None
    r2max = 0.0
    nz = tot = 0
    for f in range(to):                      # frame placement by t_mul / t_add / split, in plain Python
        for sub, lo, hi in ((0, 0, split if split > 0 else cout), (1, split, cout if split > 0 else split)):
            if hi <= lo:
                continue
            fr = f * t_mul + t_add + sub
            assert 0 <= fr < y_t and fr not in c.get("keep", ())
            v = r1[:, lo:hi, f].permute(0, 2, 3, 1)
            if res is not None:
                rr = torch.randint(-8, 9, v.shape, generator=g).double()
                res[:, fr, :, :, :hi - lo] = rr.to(BF16)
                v = v + rr
            assert not bool(written[:, fr, :, :, :hi - lo].any())
            want[:, fr, :, :, :hi - lo] = v.to(BF16)
            written[:, fr, :, :, :hi - lo] = True
            r2max = max(r2max, v.abs().max().item())
            nz += int((v != 0).sum())
            tot += v.numel()
    x = x64.to(BF16)
    x[:, :t_lo] = float("nan")
    pre = {"r1_max": r1.abs().max().item(), "r2_max": r2max, "acc_max": acc.abs().max().item(), "nonzero": nz / max(tot, 1)}
    out = dict(case=c, x=x, w=w64.to(BF16), bias=bias64.to(BF16), res=res, want=want, written=written, pre=pre, ldy=ldy)
    _CONV_CACHE[name] = out
    return out


def conv_exact_preconditions(p):
    """From the float64 reference alone: bf16(acc + bias) and bf16(that + res) exact (integers within
    +-256), and at least half of the outputs non-zero."""
    pre = p["pre"]
    assert pre["r1_max"] <= CONV_EXACT_LIMIT and pre["r2_max"] <= CONV_EXACT_LIMIT, pre
    assert pre["nonzero"] >= CONV_MIN_NONZERO, pre
    return pre


# ---------------------------------------------------------------------- VAE attention (vs_vae_attention)
# The contract of csrc/vae_attention.hip: s = fp32(q . k) * sc, sc = fp32(log2 e) / sqrtf(C); two passes,
# P = bf16(exp2(s - m) * (1 / l)), fp32 accumulation of P V, bf16 output.  Two references
# (test_vae_attention_exact_gpu.py, preconditions in test_kernel_refs_cpu.py):
#   * "tied groups": every key has a group id, every query selects one group; Q and K carry the id's
#     bits as +-a over all C dimensions (dimension d carries bit d % VATT_NB with a seeded sign on both).
#     A tied key's score exceeds every other key's by >= VATT_MIN_GAP in the exp2 domain, so exp2 of
#     every other key is exactly 0, of a tied key exactly 1, every rescale factor 0 or 1, the row sum
#     the group size g, P = bf16(fl32(1 / g)); V holds integers in -8..8, so p * sum_{j in G} V_j is
#     exact in fp32 in any order: the answer is known to the bit, with no ambiguous set;
#   * random inputs with the per-element bound 2^-8 (|o| + A), A = sum p |v| (vatt_within).
VATT_ROWS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257]
VATT_C = [128, 256, 384]
VATT_G = [1, 2, 3, 5, 7, 32, "rows"]
VATT_NZ = 2
VATT_AMP = 16.0
VATT_NB = 10                # id bits: 258 groups at most; 10 does not divide the 8-element chunks
VATT_MIN_GAP = 160.0        # exp2(-160) is below the smallest fp32 denormal
VATT_WINDOW = 8             # fp32 ulps between fl32(1 / g) and a bf16 midpoint: the device's 1 / l may be 1 ulp off
VATT_BOUND = 2.0 ** -8
# test_vae_attention_vs_float64's random cases without the 6240-row one, plus qscale 16: (c, rows, nz, ld_pad, qscale)
VATT_BOUND_CASES = [(384, 100, 3, 0, 1.0), (384, 33, 2, 64, 4.0), (384, 1, 2, 0, 1.0), (256, 31, 2, 8, 1.0),
                    (128, 1000, 2, 0, 1.0), (128, 257, 1, 0, 16.0), (384, 100, 3, 0, 16.0)]


def vatt_sc(c):
    """The kernel's score scale: fp32(log2 e) / sqrtf(C), in fp32."""
    return (torch.tensor(1.4426950408889634, dtype=torch.float32) / torch.sqrt(torch.tensor(float(c), dtype=torch.float32))).item()


def vatt_exact_inputs(rows, c, g, nz=VATT_NZ):
    """qkv [nz, rows, 3c] bf16 (CPU) of the tied-groups problem with group size g ("rows": Q = 0, every
    key ties).  g < rows: G = rows // g groups of exactly g keys, key j in group j % G (members straddle
    every key-tile boundary), the rows - G g keys left over a last, smaller group; every query selects a
    seeded group."""
    gen = torch.Generator().manual_seed(rows * 1009 + c * 7 + (0 if g == "rows" else g))
    every = g == "rows" or g >= rows
    gsz = 7 if every else g
    G = max(1, rows // gsz)
    j = torch.arange(rows)
    gid = torch.where(j < G * gsz, j % G, torch.full_like(j, G))
    ngroups = int(gid.max()) + 1
    assert ngroups <= 2 ** VATT_NB
    d = torch.arange(c)
    sigma = torch.randint(0, 2, (c,), generator=gen).double() * 2 - 1

    def carry(ids):
        bit = (ids.view(-1, 1) >> (d % VATT_NB).view(1, -1)) & 1
        return VATT_AMP * sigma.view(1, -1) * (2.0 * bit.double() - 1)
    qkv = torch.empty(nz, rows, 3 * c, dtype=torch.float64)
    for z in range(nz):
        sel = torch.randint(0, ngroups, (rows,), generator=gen)
        qkv[z, :, :c] = 0.0 if every else carry(sel)
        qkv[z, :, c:2 * c] = carry(gid)
        qkv[z, :, 2 * c:] = torch.randint(-8, 9, (rows, c), generator=gen).double()
    return qkv.to(BF16)


def vatt_exact_ref(qkv, c):
    """(ref bf16 [nz, rows, c], pre) from float64 alone.  pre: min_gap (the smallest gap, times sc, between
    a query's top score and any other key; inf when every key ties), sizes (the tie counts that occur),
    midpoint_ok (fl32(1 / g) >= VATT_WINDOW fp32 ulps from a bf16 midpoint for each), exact (p * S fits fp32)."""
    q, k, v = (qkv[..., i * c:(i + 1) * c].double() for i in range(3))
    s = q @ k.transpose(-1, -2)
    top = s.max(dim=-1, keepdim=True).values
    tie = s == top
    others = torch.where(tie, torch.full_like(s, -float("inf")), s).max(dim=-1).values
    gap = (top.squeeze(-1) - others) * vatt_sc(c)
    cnt = tie.sum(dim=-1, keepdim=True).double()
    inv = 1.0 / cnt
    p = inv.float().to(BF16).double()                        # bf16(fl32(1 / g))
    S = tie.double() @ v
    o = p * S
    pre = {"min_gap": gap.min().item(), "sizes": sorted(int(x) for x in cnt.unique()),
           "midpoint_ok": not bool(near_bf16_midpoint(inv, VATT_WINDOW).any()),
           "exact": bool((o.float().double() == o).all()) and bool((s.float().double() == s).all()),
           "nonzero": (o != 0).double().mean().item()}
    return o.float().to(BF16), pre


def vatt_exact_preconditions(pre, rows, g):
    assert pre["min_gap"] >= VATT_MIN_GAP and pre["midpoint_ok"] and pre["exact"], pre
    if g == "rows" or g >= rows:
        assert pre["sizes"] == [rows], pre
    else:
        assert set(pre["sizes"]) <= {g, rows % g} and g in pre["sizes"], pre


def vatt_buffers(qkv, c, ld_pad=8, ldo_pad=4, device="cuda"):
    """The guarded layout of one call: qkv rows of 3c + ld_pad columns with NaN in the pad columns and one
    NaN guard row after each frame; out a sentinel buffer [nz + 1, rows + 1, c + ldo_pad] (pad columns, one
    guard row per frame, one guard frame behind the last).  Returns (qbuf, out, the call's arguments after
    the pointers: qkv_zs, ld_qkv, o_zs, ld_o)."""
    nz, rows, _ = qkv.shape
    ld, ldo = 3 * c + ld_pad, c + ldo_pad
    qbuf = sentinel((nz, rows + 1, ld), device="cpu")
    qbuf[:, :rows, :3 * c] = qkv
    return qbuf.to(device), sentinel((nz + 1, rows + 1, ldo), device=device), ((rows + 1) * ld, ld, (rows + 1) * ldo, ldo)


def vatt_guards_untouched(out, rows, c):
    """Pad columns, every frame's guard row and the guard frame still hold the sentinel."""
    return untouched(out[..., c:]) and untouched(out[:, rows]) and untouched(out[-1])


def vatt_random_inputs(c, rows, nz, qscale):
    """test_vae_attention_vs_float64's inputs (N(0, 1), q scaled by qscale), seeded on the CPU."""
    g = torch.Generator().manual_seed(c + rows + int(qscale))
    x = torch.randn((nz, rows, 3 * c), generator=g)
    x[..., :c] *= qscale
    return x.to(BF16)


def vatt_ref64(qkv, c):
    """(o, A) in float64: o = softmax(q k^T / sqrt(c)) v, A = sum p |v|."""
    q, k, v = (qkv[..., i * c:(i + 1) * c].double() for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(c), dim=-1)
    return p @ v, p @ v.abs()


def vatt_within(got, o, A):
    """error / bound per element, bound = 2^-8 (|o| + A): half a bf16 ulp on each p moves the sum by at most
    2^-9 A, the output rounding by 2^-9 |o|; the rest is slack for the fp32 sums and the 1 / l reciprocal."""
    return (got.double().cpu() - o).abs() / torch.clamp(VATT_BOUND * (o.abs() + A), min=1e-300)


def vatt_emulate_fp32(qkv, c, twice_last=False, drop_key=None, shift_v=False):
    """The two-pass kernel in fp32 on the CPU, its bf16 P included: s = fl32(q . k) * sc, m = row max,
    l = sum exp2(s - m), P = bf16(exp2(s - m) * (1 / l)), out = bf16(P V).  Mutations: the last key counted
    twice, key drop_key left out, V rows shifted by one (key j weighted onto V[j + 1], cyclically)."""
    q, k, v = (qkv[..., i * c:(i + 1) * c].float() for i in range(3))
    if twice_last:
        k, v = torch.cat([k, k[:, -1:]], dim=1), torch.cat([v, v[:, -1:]], dim=1)
    if drop_key is not None:
        keep = [j for j in range(k.shape[1]) if j != drop_key]
        k, v = k[:, keep], v[:, keep]
    if shift_v:
        v = torch.roll(v, -1, dims=1)
    s = (q @ k.transpose(-1, -2)) * torch.tensor(vatt_sc(c), dtype=torch.float32)
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp2(s - m)
    p = (e * (1.0 / e.sum(dim=-1, keepdim=True))).to(BF16).float()
    return (p @ v).to(BF16)
