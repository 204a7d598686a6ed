"""The batched plain-GEMM mode of vs_vae_conv (vstyler.vae.batched_gemm): the MFMA path under the UMT5
encoder's QK^T / P.V and the VAE attention's GEMM route -- nz slices with z-strides, fp32 output with
alpha, every launch_conv<NB> pick.

Operands in {-1, 0, 1} keep every fp32 sum exact (bf16 output exact too for K <= 128), so the result
must equal the integer product bit for bit.  What the kernel guarantees outside the n_out columns of
the `rows` rows of each slice (read from conv_store in csrc/vae.hip: channels n >= cout are skipped and
a partial 4-channel group is stored element by element): UNCHANGED -- asserted here with a NaN
sentinel in columns n_out..ldy-1, in a guard row after each slice and behind the last slice.  The
operands' columns k..ld-1 hold NaN: the kernel must never let them in."""
import pytest
import torch

import gpu_util as U
from gpu_util import BF16

pytestmark = pytest.mark.gpu


def _tri(shape, g):
    return torch.randint(-1, 2, shape, generator=g).to(BF16)


def _padded(t, ld):
    """t [nz, r, k] on the device as [nz, r, ld] with NaN in columns k..ld-1; returns the [.., :k] view."""
    nz, r, k = t.shape
    buf = U.sentinel((nz, r, ld))
    buf[:, :, :k] = t.cuda()
    return buf[:, :, :k]


CASES = [
    # rows, k, n_out, nz, out_f32, alpha
    (1, 32, 16, 1, False, 1.0),         # launch_conv<1>
    (127, 64, 64, 4, False, 1.0),       # <2>
    (128, 96, 96, 1, False, 1.0),       # <3> (cout <= 96)
    (129, 512, 100, 4, True, 1.0),      # 100: padding to 128 (28) < to 192 (92) -> <4>; K = 512 exact in fp32
    (300, 64, 128, 1, False, 1.0),      # <4>, three 128-row blocks (two pixel blocks per wave + a tail)
    (300, 96, 200, 4, True, 0.125),     # two 128-channel tiles, alpha a power of two: still exact
    (129, 32, 200, 1, False, 1.0),
    (1, 512, 16, 4, True, 1.0),
    (129, 64, 192, 4, False, 1.0),      # 192: padding to 192 (0) < to 256 (64) -> <3>, two channel tiles
    (127, 128, 98, 1, False, 1.0),      # 98: a partial 4-channel group (element stores), K = 128 still exact in bf16
]


@pytest.mark.parametrize("rows,k,n_out,nz,out_f32,alpha", CASES)
def test_batched_gemm_integer_exact(rows, k, n_out, nz, out_f32, alpha):
    from vstyler import vae
    g = torch.Generator().manual_seed(rows * 1000 + k + n_out)
    a, b = _tri((nz, rows, k), g), _tri((nz, n_out, k), g)
    ref = torch.einsum("zrk,znk->zrn", a.double(), b.double()) * alpha
    assert out_f32 or k <= 128
    a_d, b_d = _padded(a, k + 8), _padded(b, k + 8)
    ldy = (n_out + 3) // 4 * 4 + 4
    odt = torch.float32 if out_f32 else BF16
    y = U.sentinel((nz, rows + 1, ldy), odt)               # a guard row per slice: y_zs = (rows + 1) * ldy
    vae.batched_gemm(a_d, a_d.stride(0), a_d.stride(1), rows, k, b_d, b_d.stride(0), b_d.stride(1), n_out,
                     y, y.stride(0), ldy, nz, out_f32=out_f32, alpha=alpha)
    torch.cuda.synchronize()
    got = y[:, :rows, :n_out].cpu()
    assert torch.equal(got.double(), ref)
    assert U.untouched(y[:, :rows, n_out:]) and U.untouched(y[:, rows:])


def test_t5_scores_layout():
    """QK^T as vstyler/t5.py launches it: A and B are the head column blocks of [L, da] matrices
    (zs = hd, ld = da), fp32 scores [nz][L][Lp] with alpha = 1; L = 100, hd = 64, nz = 4."""
    from vstyler import vae
    L, hd, nz = 100, 64, 4
    da, Lp = nz * hd, U.ceil32(L)
    g = torch.Generator().manual_seed(5)
    q, kk = _tri((L, da), g), _tri((L, da), g)
    s = U.sentinel((nz + 1, L, Lp), torch.float32)
    vae.batched_gemm(q.cuda(), hd, da, L, hd, kk.cuda(), hd, da, L, s, L * Lp, Lp, nz, out_f32=True, alpha=1.0)
    torch.cuda.synchronize()
    ref = torch.einsum("izc,jzc->zij", q.view(L, nz, hd).double(), kk.view(L, nz, hd).double())
    assert torch.equal(s[:nz, :, :L].cpu().double(), ref)
    assert U.untouched(s[:nz, :, L:]) and U.untouched(s[nz:])


def test_t5_pv_layout():
    """P.V as vstyler/t5.py launches it: A = P [nz][L][Lp] read over K = Lp = 128 (its pad columns are the
    zeros vs_t5_bias_softmax writes), B = V^T [nz][hd][Lp] (pad columns the zeros vs_vae_transpose
    writes), bf16 output into the head column blocks of [L, da] (y_zs = hd, ldy = da)."""
    from vstyler import vae
    L, hd, nz = 100, 64, 4
    da, Lp = nz * hd, U.ceil32(L)
    g = torch.Generator().manual_seed(6)
    p, vt = torch.zeros(nz, L, Lp, dtype=BF16), torch.zeros(nz, hd, Lp, dtype=BF16)
    p[:, :, :L], vt[:, :, :L] = _tri((nz, L, L), g), _tri((nz, hd, L), g)
    o = U.sentinel((L + 1, da))
    vae.batched_gemm(p.cuda(), L * Lp, Lp, L, Lp, vt.cuda(), hd * Lp, Lp, hd, o, hd, da, nz)
    torch.cuda.synchronize()
    ref = torch.einsum("zij,zcj->izc", p.double(), vt.double()).reshape(L, da)
    assert torch.equal(o[:L].cpu().double(), ref)
    assert U.untouched(o[L:])


def test_batched_gemm_random_fp32():
    """N(0, 1) operands, fp32 output, against float64: |got - ref| <= (K + 2) 2^-24 sum_k |a_k b_k| per
    element (the standard bound of an fp32 accumulation in any order)."""
    from vstyler import vae
    rows, k, n_out, nz = 129, 512, 100, 2
    g = torch.Generator().manual_seed(7)
    a, b = torch.randn(nz, rows, k, generator=g).to(BF16), torch.randn(nz, n_out, k, generator=g).to(BF16)
    a_d, b_d = _padded(a, k + 8), _padded(b, k + 8)
    y = U.sentinel((nz, rows + 1, n_out + 4), torch.float32)
    vae.batched_gemm(a_d, a_d.stride(0), a_d.stride(1), rows, k, b_d, b_d.stride(0), b_d.stride(1), n_out,
                     y, y.stride(0), y.stride(1), nz, out_f32=True, alpha=1.0)
    torch.cuda.synchronize()
    ref = torch.einsum("zrk,znk->zrn", a.double(), b.double())
    mag = torch.einsum("zrk,znk->zrn", a.double().abs(), b.double().abs())
    d = (y[:, :rows, :n_out].cpu().double() - ref).abs()
    bound = (k + 2) * 2.0 ** -24 * mag
    print(f"batched_gemm random: max |got - ref| / bound = {(d / bound).max().item():.4f}")
    assert bool((d <= bound).all())
    assert U.untouched(y[:, :rows, n_out:]) and U.untouched(y[:, rows:])
