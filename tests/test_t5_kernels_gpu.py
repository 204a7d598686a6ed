"""Direct parity of the UMT5 encoder's own kernels (csrc/t5.hip) against plain references:
vs_embed_rows, vs_t5_bias_softmax, vs_t5_gelu_mul -- the shapes test_t5_gpu.py never reaches
(L not a multiple of 32: the zeroed pad columns of P; head slices; every mask shape) and every bf16
input of the GELU chain.  Output buffers are pre-filled with a NaN sentinel and everything outside the
documented output region must keep it; unread input pads hold NaN."""
import pytest
import torch

from oracle import t5_oracle as T
import gpu_util as U
from gpu_util import BF16

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dim", [8, 256, 4096])    # one 16-B vector / a partial pass / two passes of 256 threads
def test_embed_rows(dim):
    vocab, pad = 1000, 16
    g = torch.Generator().manual_seed(dim)
    # the table is a column slice of a wider buffer (ld_table > dim); every bit pattern may occur
    wide = torch.randint(-32768, 32768, (vocab, dim + pad), generator=g, dtype=torch.int32).to(torch.int16).view(BF16)
    wide = wide.cuda()
    table = wide[:, 8:8 + dim]
    ids = torch.tensor([0, vocab - 1, 5, 5, 0, vocab - 1, 123, 998, 1, 5, 777], dtype=torch.int64)
    rows = ids.numel()
    ids_d = ids.cuda()
    out = U.sentinel((rows + 1, dim + 8))
    U.call("vs_embed_rows", ids_d.data_ptr(), table.data_ptr(), table.stride(0), vocab, out.data_ptr(),
           out.stride(0), rows, dim, U.stream())
    torch.cuda.synchronize()
    assert U.same_bits(out[:rows, :dim].contiguous(), table[ids_d].contiguous())
    assert U.untouched(out[:rows, dim:]) and U.untouched(out[rows:])


def _masks(L):
    ones = torch.ones(L, dtype=torch.int32)
    out = {"ones": ones}
    for name, n in (("prefix1", 1), ("prefixL-1", L - 1)):
        m = torch.zeros(L, dtype=torch.int32)
        m[:n] = 1
        out[name] = m
    holes = (torch.arange(L) % 3 != 1).to(torch.int32)
    holes[L // 2:L // 2 + 2] = 0
    holes[0] = 1
    out["holes"] = holes
    out["zero"] = torch.zeros(L, dtype=torch.int32)
    return out


@pytest.mark.parametrize("L,tight", [(1, False), (17, False), (64, False), (65, False), (100, False), (512, False),
                                     (100, True)])
def test_t5_bias_softmax(L, tight):
    """Against the oracle's expression (t5_attention): bf16(s) + bf16 bias (finfo.min on masked keys) as a
    bf16 tensor op, softmax in float64.  |got - ref| <= 2^-8 ref + 1e-30: one bf16 ulp (half an ulp of
    rounding + the fp32 expf / division error) -- derived, not measured.  Pad columns L..ld_p-1 and
    masked columns are +0 bit for bit whenever the row has a valid key; with every key masked every
    score is finfo.min, exp(0) = 1 and the sum is exactly L, so each valid column is exactly bf16(1/L)."""
    nheads, nbuckets = 4, 32
    ld_s = U.ceil32(L)
    ld_p = L if tight else U.ceil32(L)
    g = torch.Generator().manual_seed(1000 + L)
    emb = (0.5 * torch.randn(nbuckets, nheads, generator=g)).to(BF16)
    buckets = T.relative_position_bucket(L, L, nbuckets).to(torch.int32)
    emb_d, buckets_d = emb.cuda(), buckets.cuda().contiguous()
    inv_l = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(L), dtype=torch.float32)).to(BF16)
    for head0, nz in ((0, 4), (1, 2), (3, 1)):
        s = 2.0 * torch.randn(nz, L, L, generator=g)                       # N(0, 4) fp32
        zs_s, zs_p = L * ld_s + 32, L * ld_p + 32                          # gaps between the slices
        s_d = U.sentinel(nz * zs_s, torch.float32)                         # NaN in the unread pad / gaps
        s_v = s_d.as_strided((nz, L, ld_s), (zs_s, ld_s, 1))
        s_v[:, :, :L] = s.cuda()
        for name, mask in _masks(L).items():
            p_d = U.sentinel(nz * zs_p + 64)
            mask_d = mask.cuda()
            U.call("vs_t5_bias_softmax", s_d.data_ptr(), zs_s, ld_s, p_d.data_ptr(), zs_p, ld_p,
                   buckets_d.data_ptr(), emb_d.data_ptr(), nheads, head0, mask_d.data_ptr(), L, nz, U.stream())
            torch.cuda.synchronize()
            p = p_d.cpu()
            pv = p.as_strided((nz, L, ld_p), (zs_p, ld_p, 1))
            tag = (L, ld_p, head0, nz, name)
            # nothing outside the nz x L x ld_p rows is written
            keep = torch.ones(p.numel(), dtype=torch.bool)
            keep.as_strided((nz, L, ld_p), (zs_p, ld_p, 1)).fill_(False)
            assert U.untouched(p[keep]), tag
            assert U.bit_zero(pv[:, :, L:]), tag
            got = pv[:, :, :L]
            if int(mask.sum()) == 0:
                assert bool((U.bits(got) == U.bits(inv_l)).all()), tag
                continue
            assert U.bit_zero(got[:, :, mask == 0]), tag
            _, ref = U.t5_softmax_ref(s, emb, buckets, mask, head0, nz)
            ok = U.softmax_within(got, ref)
            assert bool(ok.all()), (tag, (got.double() - ref).abs().max().item())


@pytest.mark.parametrize("inplace", [False, True])
def test_t5_gelu_mul_every_bf16(inplace):
    """g over every bf16 bit pattern: bit-identical to bf16(a * gelu_bf16(g)) except where the float64
    tanh lies within 4 fp32 ulps of a bf16 rounding midpoint (from the reference alone; there within 2
    bf16 ulps).  inplace: out == a, as vstyler/t5.py calls it."""
    a, g = U.t5_gelu_inputs()
    n = a.numel()
    assert n % 256 != 0
    ref, amb = U.t5_gelu_mul_ref(a, g)
    print(f"t5_gelu_mul: ambiguous share {amb.double().mean().item():.6f} ({int(amb.sum())} of {n})")
    assert amb.double().mean().item() <= 0.01
    tail = 27
    buf = U.sentinel(n + tail)
    a_d, g_d = a.cuda(), g.cuda()
    if inplace:
        buf[:n] = a_d
        src = buf
    else:
        src = a_d
    U.call("vs_t5_gelu_mul", src.data_ptr(), g_d.data_ptr(), buf.data_ptr(), n, U.stream())
    torch.cuda.synchronize()
    got = buf[:n].cpu()
    assert U.untouched(buf[n:])
    same = U.same_bits_or_nan(got, ref)
    bad = ~same & ~amb
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} non-ambiguous elements differ; first g bits "
                             f"{int(U.bits(g)[i]) & 0xffff:#06x} a {a[i].item()} got {got[i].item()} ref {ref[i].item()}")
    loose = amb & ~same
    if bool(loose.any()):
        dist = (U.bf16_ord(got) - U.bf16_ord(ref)).abs()[loose]
        assert torch.isfinite(got[loose].float()).all() and int(dist.max()) <= 2, int(dist.max())
