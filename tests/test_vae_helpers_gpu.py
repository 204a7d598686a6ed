"""Direct parity of the VAE's helper kernels (csrc/vae.hip): vs_vae_softmax, vs_vae_transpose,
vs_vae_tile_gather, vs_vae_tile_blend + vs_vae_blend_finish, vs_vae_copy_frames -- until now reached
only through whole encode / decode comparisons within the oracle's floor.  Outputs are pre-filled with
a NaN sentinel (everything outside the documented region must keep it), documented pads must be +0 bit
for bit, unread input pads hold NaN, and wherever the header promises the reference's bf16 arithmetic
the comparison is of bit patterns."""
import pytest
import torch

from oracle import wan_vae_oracle as V
import gpu_util as U
from gpu_util import BF16

pytestmark = pytest.mark.gpu


def _bf(x):
    return x.to(BF16)


@pytest.mark.parametrize("ncols", [1, 63, 64, 65, 600])
def test_vae_softmax(ncols):
    """Row softmax of fp32 scores against float64, |got - ref| <= 2^-8 ref + 1e-30 (one bf16 ulp: half an
    ulp of rounding + the fp32 expf / reciprocal error); one row offset by +1e4 overflows without the
    max subtraction; pad columns ncols..ld_p-1 are +0."""
    rows, ld = 7, U.ceil32(ncols)
    g = torch.Generator().manual_seed(ncols)
    s = 2.0 * torch.randn(rows, ncols, generator=g)
    s[3] += 1e4
    s_d = U.sentinel((rows, ld), torch.float32)
    s_d[:, :ncols] = s.cuda()
    p = U.sentinel((rows + 1, ld))
    U.call("vs_vae_softmax", s_d.data_ptr(), ld, p.data_ptr(), ld, rows, ncols, U.stream())
    torch.cuda.synchronize()
    ref = torch.softmax(s.double(), dim=-1)
    got = p[:rows, :ncols].cpu()
    assert bool(U.softmax_within(got, ref).all()), (got.double() - ref).abs().max().item()
    assert U.bit_zero(p[:rows, ncols:]) and U.untouched(p[rows:])


@pytest.mark.parametrize("layout", ["t5", "vae"])
def test_vae_transpose(layout):
    """vt[z][c][r] = v[z][r][c], columns rows..ld_vt-1 written +0, in both product layouts: the UMT5 one
    (v the head column blocks of [rows, nz * cols]: v_zs = cols, ld_v = nz * cols) and the VAE one (v the
    third column block of [nz][rows][3c]: v_zs = rows * 3c, ld_v = 3c)."""
    nz = 3
    g = torch.Generator().manual_seed(11)
    for rows in (1, 31, 33, 100):
        for cols in (1, 32, 40, 64, 384):
            if layout == "t5":
                src = torch.randn(rows, nz * cols, generator=g).to(BF16).cuda()
                v, v_zs, ld_v = src, cols, nz * cols
                want = src.view(rows, nz, cols).permute(1, 2, 0)
            else:
                src = torch.randn(nz, rows, 3 * cols, generator=g).to(BF16).cuda()
                v, v_zs, ld_v = src[0, :, 2 * cols:], rows * 3 * cols, 3 * cols
                want = src[:, :, 2 * cols:].permute(0, 2, 1)
            ld_vt = U.ceil32(rows)
            vt_zs = cols * ld_vt + 32                       # a gap after every slice
            vt = U.sentinel(nz * vt_zs)
            U.call("vs_vae_transpose", v.data_ptr(), v_zs, ld_v, vt.data_ptr(), vt_zs, ld_vt, nz, rows, cols,
                   U.stream())
            torch.cuda.synchronize()
            view = vt.as_strided((nz, cols, ld_vt), (vt_zs, ld_vt, 1))
            assert U.same_bits(view[:, :, :rows].contiguous(), want.contiguous()), (rows, cols)
            assert U.bit_zero(view[:, :, rows:]), (rows, cols)
            assert U.untouched(vt.as_strided((nz, 32), (vt_zs, 1), cols * ld_vt)), (rows, cols)


def _affine_ref(x, mode, a, b):
    """The header's order on bf16 tensors: mode 1 bf16(bf16(x - a) * b), mode 2 bf16(bf16(x / b) + a);
    a, b broadcast over the last (channel) dim."""
    if mode == 1:
        return _bf(_bf(x.float() - a.float()).float() * b.float())
    if mode == 2:
        return _bf(_bf(x.float() / b.float()).float() + a.float())
    return x


def _ab(c, g):
    a = torch.randn(c, generator=g).to(BF16)
    b = ((0.5 + torch.rand(c, generator=g)) * (1 - 2 * (torch.arange(c) % 2))).to(BF16)    # |b| >= 0.5
    return a, b


@pytest.mark.parametrize("C", [3, 16])
def test_vae_tile_gather(C):
    """Tile cut of NCTHW into an NTHWC tile with zero pad channels and the per-channel affine modes,
    bit for bit; tiles at the origin, in the interior and at the far corner (h0 + th = h, w0 + tw = w).
    An odd cpad (C + 1 = 17) is rejected by the host check (VS_E_INVALID) with nothing written."""
    t_src, t, H, W, th, tw = 3, 2, 12, 20, 5, 7
    g = torch.Generator().manual_seed(C)
    src = torch.randn(C, t_src, H, W, generator=g).to(BF16)
    a, b = _ab(C, g)
    src_d, a_d, b_d = src.cuda(), a.cuda(), b.cuda()
    for cpad in (C + 1, 32):
        for h0, w0 in ((0, 0), (3, 4), (H - th, W - tw)):
            for mode in (0, 1, 2):
                n = t * th * tw * cpad
                dst = U.sentinel(n + 16)
                rc = U.call_rc("vs_vae_tile_gather", src_d.data_ptr(), C, t_src, H, W, t, h0, w0, th, tw,
                               dst.data_ptr(), cpad, mode, a_d.data_ptr() if mode else None,
                               b_d.data_ptr() if mode else None, U.stream())
                torch.cuda.synchronize()
                if cpad % 2:
                    assert rc == 1 and U.untouched(dst)
                    continue
                assert rc == 0
                cut = src[:, :t, h0:h0 + th, w0:w0 + tw].permute(1, 2, 3, 0)         # [t, th, tw, C]
                ref = _affine_ref(cut, mode, a, b)
                tile = dst[:n].view(t, th, tw, cpad)
                assert U.same_bits(tile[..., :C].contiguous(), ref.contiguous()), (cpad, h0, w0, mode)
                assert U.bit_zero(tile[..., C:]) and U.untouched(dst[n:]), (cpad, h0, w0, mode)


@pytest.mark.parametrize("H", [24, 32])     # 2 x 2 and 3 x 2 tiles (32: a middle tile row ramped on both sides)
@pytest.mark.parametrize("mode", [0, 2])
def test_vae_tile_blend_and_finish(H, mode):
    """Overlapping 16 x 24 tiles at stride 8 x 16 over H x 40, t = 2, c = 3, blended in V.tile_tasks order
    with V.build_mask masks in bf16 exactly as V.tiled_decode accumulates: values and weight bit for bit
    after every tile, then bf16(values / weight) with and without the clamp.  mode 2: the tile's
    de-normalisation applied first."""
    Wd, size, stride, t, c, ldc = 40, (16, 24), (8, 16), 2, 3, 4
    tasks = V.tile_tasks(H, Wd, size, stride)
    assert len(tasks) == (H // 8 - 1) * 2
    g = torch.Generator().manual_seed(H + mode)
    a, b = _ab(c, g)
    a_d, b_d = a.cuda(), b.cuda()
    plane = t * H * Wd
    vals = U.sentinel(c * plane + 8)
    wgt = U.sentinel(plane + 8)
    vals[:c * plane] = 0
    wgt[:plane] = 0
    ref_v = torch.zeros(c, t, H, Wd, dtype=BF16)
    ref_w = torch.zeros(t, H, Wd, dtype=BF16)
    bw = (size[0] - stride[0], size[1] - stride[1])
    for h, h_, w, w_ in tasks:
        th, tw = size
        tile = U.sentinel((t, th, tw, ldc), device="cpu")                  # channel 3: an unread pad
        tile[..., :c] = (1.5 * torch.randn(t, th, tw, c, generator=g)).to(BF16)
        is_bound = (h == 0, h_ >= H, w == 0, w_ >= Wd)
        bound = int(is_bound[0]) | int(is_bound[1]) << 1 | int(is_bound[2]) << 2 | int(is_bound[3]) << 3
        tile_d = tile.cuda()
        U.call("vs_vae_tile_blend", tile_d.data_ptr(), ldc, c, t, th, tw, vals.data_ptr(), wgt.data_ptr(),
               H, Wd, h, w, bound, bw[0], bw[1], mode, a_d.data_ptr() if mode else None,
               b_d.data_ptr() if mode else None, U.stream())
        torch.cuda.synchronize()
        mask = V.build_mask(th, tw, is_bound, bw).to(BF16).view(1, th, tw)
        v = _affine_ref(tile[..., :c], mode, a, b).permute(3, 0, 1, 2)      # [c, t, th, tw]
        rv, rw = ref_v[:, :, h:h_, w:w_], ref_w[:, h:h_, w:w_]
        rv.copy_(_bf(rv.float() + _bf(v.float() * mask.float()).float()))
        rw.copy_(_bf(rw.float() + mask.float()))
        assert U.same_bits(vals[:c * plane].view_as(ref_v), ref_v), (h, w)
        assert U.same_bits(wgt[:plane].view_as(ref_w), ref_w), (h, w)
        assert U.untouched(vals[c * plane:]) and U.untouched(wgt[plane:])
    assert float(ref_w.float().min()) > 0
    quot = _bf(ref_v.float() / ref_w.float())
    assert float(quot.float().abs().max()) > 1                              # the clamp has something to do
    for clamp in (0, 1):
        out = U.sentinel(c * plane + 8)
        U.call("vs_vae_blend_finish", vals.data_ptr(), wgt.data_ptr(), out.data_ptr(), c, plane, clamp, U.stream())
        torch.cuda.synchronize()
        ref = quot.clamp(-1, 1) if clamp else quot
        assert U.same_bits(out[:c * plane].view_as(ref), ref), clamp
        assert U.untouched(out[c * plane:])


def test_vae_copy_frames():
    """vs_vae_copy_frames through vae.copy_first_frame (the pass-through first frame of Resample) and
    directly with source and destination strides larger than the copied plane: bit for bit, the
    neighbours unchanged."""
    from vstyler import vae
    g = torch.Generator().manual_seed(3)
    n, t, h, w, c = 2, 3, 4, 5, 8
    src = torch.randn(n, t, h, w, c, generator=g).to(BF16).cuda()
    dst = U.sentinel((n, 5, h, w, c))
    vae.copy_first_frame(src, dst)
    torch.cuda.synchronize()
    assert U.same_bits(dst[:, 0].contiguous(), src[:, 0].contiguous()) and U.untouched(dst[:, 1:])
    nn, fe, src_ns, dst_ns = 3, 70, 100, 90
    s2 = torch.randn(nn * src_ns, generator=g).to(BF16).cuda()
    d2 = U.sentinel(nn * dst_ns + 10)
    U.call("vs_vae_copy_frames", s2.data_ptr(), src_ns, d2.data_ptr(), dst_ns, nn, fe, U.stream())
    torch.cuda.synchronize()
    dv = d2[:nn * dst_ns].view(nn, dst_ns)
    assert U.same_bits(dv[:, :fe].contiguous(), s2.view(nn, src_ns)[:, :fe].contiguous())
    assert U.untouched(dv[:, fe:]) and U.untouched(d2[nn * dst_ns:])
