"""The sampler / elementwise entries at the sizes, modes and operand layouts the model-level tests never
reach: vs_axpy, vs_cast, vs_cfg_euler[_dev] without CFG, vs_mod_add in the head's layout,
vs_time_sinusoid over every timestep, vs_patchify / vs_unpatchify at VACE's 96 channels, every mode of
vs_unipc_update.  All bit for bit against the oracle's expressions as separate torch ops; outputs are
pre-filled with a NaN sentinel and the neighbours of the output region must keep it."""
import ctypes

import pytest
import torch

from oracle import wan_oracle as O
import gpu_util as U
from gpu_util import BF16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from vstyler import kernels
    return kernels


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


@pytest.mark.parametrize("n", [8, 8 * 773])
@pytest.mark.parametrize("scale", [1.0, 0.975, -0.5, 0.0])
def test_axpy(K, n, scale):
    """x = bf16(x + bf16(y * scale)) on 16-B-aligned interior slices; the neighbours keep the sentinel."""
    g = torch.Generator().manual_seed(n)
    x, y = torch.randn(n, generator=g).to(BF16), (3.0 * torch.randn(n, generator=g)).to(BF16)
    ref = O.bf(x.float() + O.bf(y.float() * _f32(scale)).float())
    xb, yb = U.sentinel(n + 32), U.sentinel(n + 24)
    xs, ys = xb[8:8 + n], yb[16:16 + n]
    xs.copy_(x.cuda())
    ys.copy_(y.cuda())
    K.axpy(xs, ys, scale)
    torch.cuda.synchronize()
    assert U.same_bits(xs, ref)
    assert U.same_bits(ys, y)
    assert U.untouched(xb[:8]) and U.untouched(xb[8 + n:])


def _cast_f32_specials():
    pats = []
    for hi in (0x3F80, 0x3F81, 0x0000, 0x0001, 0x007F, 0x0080, 0x7F7F, 0x7F00, 0x4049, 0x8000, 0xBF80, 0xBF81, 0xFF7F):
        for lo in (0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF):     # exact ties (above even / odd), around them
            pats.append((hi << 16) | lo)
    pats += [0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345,   # +-inf, NaNs
             0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,                           # round up to +-inf
             0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80000001, 0x807F8000]   # fp32 denormals
    t = torch.tensor(pats, dtype=torch.int64)
    return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)


@pytest.mark.parametrize("n", [1, 257, 65537])
def test_cast(n):
    """vs_cast against torch's .to(): bf16 -> fp32 over every bit pattern (n = 65 537), fp32 -> bf16
    (round to nearest even) on exact ties above even and odd neighbours, +-inf, NaN, values that round
    up to inf and denormals, repeated to n elements.  Bitwise; NaN compares as NaN."""
    src16 = (torch.arange(n, dtype=torch.int32) * (1 if n > 257 else 255)).to(torch.int16).view(BF16)
    dst = U.sentinel(n + 5, torch.float32)
    s_d = src16.cuda()
    U.call("vs_cast", s_d.data_ptr(), dst.data_ptr(), n, 0, U.stream())
    torch.cuda.synchronize()
    assert bool(U.same_bits_or_nan(dst[:n], src16.float()).all()) and U.untouched(dst[n:])
    sp = _cast_f32_specials()
    g = torch.Generator().manual_seed(n)
    rnd = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    src32 = torch.cat([sp, rnd])[:n] if n > 1 else sp[:1]
    src32 = src32.view(torch.float32)
    dst = U.sentinel(n + 5)
    s_d = src32.cuda()
    U.call("vs_cast", s_d.data_ptr(), dst.data_ptr(), n, 1, U.stream())
    torch.cuda.synchronize()
    ref = src32.to(BF16)
    ok = U.same_bits_or_nan(dst[:n], ref)
    assert bool(ok.all()), [hex(int(v) & 0xFFFFFFFF) for v in U.bits(src32)[~ok][:8]]
    assert U.untouched(dst[n:])


@pytest.mark.parametrize("n", [8, 8 * 257])
@pytest.mark.parametrize("cfg", [None, 1.0, 1.2, 5.0])        # None: use_cfg = 0 with v_neg = None
def test_cfg_euler_and_dev(K, n, cfg):
    g = torch.Generator().manual_seed(n + 1)
    vp, vn, x = (torch.randn(n, generator=g).to(BF16) for _ in range(3))
    ds = O.euler_delta(O.set_timesteps(7)[0], 2)                # a 0-d fp32 tensor with a full mantissa
    if cfg is None:
        ref = O.bf(x.float() + O.bf(vp.float() * ds).float())
    else:
        ref = O.cfg_euler(vp, vn, x, cfg, ds)
    vn_d = None if cfg is None else vn.cuda()
    xb = U.sentinel(n + 16)
    x1 = xb[8:8 + n]
    x1.copy_(x.cuda())
    K.cfg_euler(vp.cuda(), vn_d, x1, cfg or 0.0, float(ds))
    x2 = x.cuda()
    K.cfg_euler_dev(vp.cuda(), vn_d, x2, cfg or 0.0, ds.reshape(1).cuda())
    torch.cuda.synchronize()
    assert U.same_bits(x1, ref) and U.same_bits(x2, ref) and U.same_bits(x1, x2)
    assert U.untouched(xb[:8]) and U.untouched(xb[8 + n:])


@pytest.mark.parametrize("rows,dim", [(6, 64), (6, 1536), (2, 1536)])
@pytest.mark.parametrize("form", ["block", "head"])
def test_mod_add(K, rows, dim, form):
    """out[b][r][d] = bf16(param[r][d] + tv[...]) in both stride forms of the model: the blocks'
    (rows * D, D) (models.py: modulation + t_mod) and the head's (D, 0) (one t row per batch broadcast
    over the rows)."""
    B = 2
    g = torch.Generator().manual_seed(rows * dim)
    p = torch.randn(rows, dim, generator=g).to(BF16)
    if form == "block":
        tv = torch.randn(B, rows, dim, generator=g).to(BF16)
        strides, ref = (rows * dim, dim), O.bf(p.float() + tv.float())
    else:
        tv = torch.randn(B, dim, generator=g).to(BF16)
        strides, ref = (dim, 0), O.bf(p.float() + tv.float().unsqueeze(1))
    buf = U.sentinel(B * rows * dim + 8)
    out = buf[:B * rows * dim].view(B, rows, dim)
    K.mod_add(p.cuda(), tv.cuda(), out, *strides)
    torch.cuda.synchronize()
    assert U.same_bits(out, ref) and U.untouched(buf[B * rows * dim:])


@pytest.mark.parametrize("dim", [2, 256])
def test_time_sinusoid_every_timestep(K, dim):
    """Every integer timestep 0..1000 and 50 fractional ones (as bf16): bit-equal to the oracle's fp64
    embedding, except elements whose float64 value lies within 4 fp64 ulps of a rounding boundary of
    the conversion (none expected; the count is printed)."""
    t = U.sinusoid_inputs()
    ref, amb = U.sinusoid_ref(dim, t)
    print(f"time_sinusoid dim {dim}: {int(amb.sum())} ambiguous of {amb.numel()}")
    buf = U.sentinel(t.numel() * dim + 8)
    out = buf[:t.numel() * dim].view(t.numel(), dim)
    K.time_sinusoid(t.cuda(), out)
    torch.cuda.synchronize()
    same = U.bits(out.cpu()) == U.bits(ref)
    assert bool((same | amb).all()), int((~same & ~amb).sum())
    assert U.untouched(buf[t.numel() * dim:])


@pytest.mark.parametrize("B,C,T,H,W", [(2, 96, 1, 4, 2), (2, 16, 2, 6, 10)])    # VACE's 96 channels at w2 = 1
def test_patchify_unpatchify_channels(K, B, C, T, H, W):
    g = torch.Generator().manual_seed(C)
    lat = torch.randn(B, C, T, H, W, generator=g).to(BF16)
    D, S = 4 * C, T * (H // 2) * (W // 2)
    buf = U.sentinel(B * S * D + 8)
    cols = buf[:B * S * D].view(B * S, D)
    K.patchify(lat.cuda(), cols)
    eye = torch.eye(D).reshape(D, C, 1, 2, 2).to(BF16)
    ref, grid = O.patchify(lat, eye, torch.zeros(D, dtype=BF16))
    torch.cuda.synchronize()
    assert U.same_bits(cols.view_as(ref), ref) and U.untouched(buf[B * S * D:])
    tok = torch.randn(B * S, D, generator=g).to(BF16)
    buf = U.sentinel(B * S * D + 8)
    back = buf[:B * S * D].view(B, C, T, H, W)
    K.unpatchify(tok.cuda(), back)
    torch.cuda.synchronize()
    assert U.same_bits(back, O.unpatchify(tok.view(B, S, D), grid, C).contiguous())
    assert U.untouched(buf[B * S * D:])


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_unipc_update_modes(mode):
    """Every mode of vs_unipc_update against the same expression as separate fp32 torch ops on the CPU
    (each op rounded, no contraction), coefficients with full mantissas, n = 1000 (a partial block)."""
    n = 1000
    g = torch.Generator().manual_seed(40 + mode)
    x, m0, m1, mt = (torch.randn(n, generator=g) for _ in range(4))
    coef = [0.8712345, 0.1234567, 0.4567891, 0.5, 0.3141592, 1.7320508]
    c1, c2, c3, r0, r1, rk = (_f32(v) for v in coef)
    if mode == 0:
        ref = x - c1 * mt
    else:
        base = c1 * x - c2 * m0
        d1 = (m1 - m0) / rk
        if mode == 1:
            ref = base
        elif mode == 2:
            ref = base - c3 * (r0 * d1)
        elif mode == 3:
            ref = base - c3 * (r1 * (mt - m0))
        else:
            ref = base - c3 * (r0 * d1 + r1 * (mt - m0))
    out = U.sentinel(n + 7, torch.float32)
    dev = {k: v.cuda() for k, v in dict(x=x, m0=m0, m1=m1, mt=mt).items()}
    U.call("vs_unipc_update", out.data_ptr(), dev["x"].data_ptr(), dev["m0"].data_ptr(), dev["m1"].data_ptr(),
           dev["mt"].data_ptr(), n, mode, (ctypes.c_float * 6)(*coef), U.stream())
    torch.cuda.synchronize()
    assert U.same_bits(out[:n], ref) and U.untouched(out[n:])


def test_ulysses_permute_entry(K):
    """vs_ulysses_permute itself (the wrapper calls vs_ulysses_permute_rows): every mode equal to the rows
    entry with packed_ld = cols_per_rank, and mode 0 equal to the plain permutation."""
    B, Sl, P, cpr = 2, 5, 3, 16
    D = P * cpr
    g = torch.Generator().manual_seed(9)
    local = torch.randn(B * Sl, D, generator=g).to(BF16).cuda()
    full = torch.randn(B * P * Sl, cpr, generator=g).to(BF16).cuda()
    n = P * B * Sl * cpr
    for mode, src in ((0, local), (3, full)):
        a, b = U.sentinel(n + 8), U.sentinel(n + 8)
        U.call("vs_ulysses_permute", src.data_ptr(), a.data_ptr(), B, Sl, P, cpr, D, B * Sl * cpr, mode, U.stream())
        K.ulysses_permute(src, b, B, Sl, P, cpr, D, B * Sl * cpr, mode)
        torch.cuda.synchronize()
        assert U.same_bits(a, b) and U.untouched(a[n:])
        if mode == 0:
            assert U.same_bits(a[:n], local.view(B, Sl, P, cpr).permute(2, 0, 1, 3).reshape(-1))
        packed = a[:n].clone()
        for back, shape in ((1, (B * Sl, D)), (2, (B * P * Sl, cpr))):
            c, d = U.sentinel(shape), U.sentinel(shape)
            U.call("vs_ulysses_permute", packed.data_ptr(), c.data_ptr(), B, Sl, P, cpr, D, B * Sl * cpr, back,
                   U.stream())
            K.ulysses_permute(packed, d, B, Sl, P, cpr, D, B * Sl * cpr, back)
            torch.cuda.synchronize()
            assert U.same_bits(c, d) and not U.untouched(c)
