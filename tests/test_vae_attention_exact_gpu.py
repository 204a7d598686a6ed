"""vs_vae_attention (csrc/vae_attention.hip) on an exact-answer tier and a derived-bound tier, with guards
around everything it reads and writes (helpers in gpu_util.py, "VAE attention"; the preconditions of
every case and the teeth of both bars in test_kernel_refs_cpu.py).

Exact tier ("tied groups"): every key has a group id and every query selects one group; Q and K carry
the id's bits as +-16 over all C dimensions (dimension d carries bit d % 10 with a seeded sign on both, so
a chunk permutation inside a K row scrambles the scores).  The smallest gap between a query's top score
and any other key, times the kernel's sc = fp32(log2 e) / sqrtf(C), is >= 160 (asserted from the float64
scores; about 780 at C = 128): exp2 of every other key is exactly 0, of a tied key exactly 1, every
rescale factor 0 or 1, the row sum the group size g as an integer, P = bf16(1 / g).  V holds integers in
-8..8, so p * sum_{j in G} V_j is exact in fp32 in any order and the answer is
bf16(fl32(bf16(fl32(1 / g))) * S).  fl32(1 / g) lies >= 8 fp32 ulps from a bf16 midpoint for every g that
occurs (asserted; the closest is 1 / 255 at 129), so the device's reciprocal cannot move P.  Bar:
bit-identical, no ambiguous set.  g in {1, 2, 3, 5, 7, 32, rows}: key j of the first G g keys is in group
j % G (members straddle every key-tile boundary); "rows" is Q = 0, every key ties -- the case that counts
keys: a mask off by one changes 1 / rows.  rows in {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257}
(key tiles of 32, query blocks of 128, both parities of nt: the ring slot of the first pass-2 tile is
nt & 1), C in {128, 256, 384}, nz = 2.

Layout of every call: ld_qkv = 3C + 8 with NaN pad columns and one NaN guard row after each frame (the
kernel clamps its reads to rows - 1); out a sentinel buffer with ld_o = C + 4, one guard row per frame and
a guard frame behind the last, all asserted untouched.

Bound tier: the random cases of test_vae_attention_gpu.py (without its 6240-row one) plus qscale 16,
|got - o| <= 2^-8 (|o| + A) per element against float64 o and A = sum p |v|: half a bf16 ulp on each p is
2^-9 A, the output rounding 2^-9 |o|, the rest slack for the fp32 sums and the 1 / l reciprocal --
derived, not measured; the worst error / bound per case is printed (DESIGN.md records it)."""
import pytest
import torch

import gpu_util as U

pytestmark = pytest.mark.gpu


def _call(qkv, c, ld_pad=8):
    """vs_vae_attention on the guarded layout; returns the whole out buffer [nz + 1, rows + 1, c + 4] (CPU)."""
    nz, rows, _ = qkv.shape
    qbuf, out, (qkv_zs, ld, o_zs, ldo) = U.vatt_buffers(qkv, c, ld_pad)
    before = U.bits(qbuf).clone()
    U.call("vs_vae_attention", qbuf.data_ptr(), qkv_zs, ld, out.data_ptr(), o_zs, ldo, nz, rows, c, U.stream())
    torch.cuda.synchronize()
    assert torch.equal(U.bits(qbuf), before)
    return out.cpu()


@pytest.mark.parametrize("rows", U.VATT_ROWS)
@pytest.mark.parametrize("c", U.VATT_C)
def test_vae_attention_tied_groups_exact(c, rows):
    for g in U.VATT_G:
        if g != "rows" and g >= rows:
            continue                                    # the same problem as "rows"
        qkv = U.vatt_exact_inputs(rows, c, g)
        ref, pre = U.vatt_exact_ref(qkv, c)
        U.vatt_exact_preconditions(pre, rows, g)        # from the float64 reference alone
        out = _call(qkv, c)
        got = out[:U.VATT_NZ, :rows, :c]
        diff = U.bits(got) != U.bits(ref)
        text = f"C {c} rows {rows} g {g}: {int(diff.sum())} of {diff.numel()} differ, sizes {pre['sizes']}"
        assert U.vatt_guards_untouched(out, rows, c), text
        assert torch.equal(U.bits(got), U.bits(ref)), text


@pytest.mark.parametrize("c,rows,nz,ld_pad,qscale", U.VATT_BOUND_CASES)
def test_vae_attention_within_derived_bound(c, rows, nz, ld_pad, qscale):
    qkv = U.vatt_random_inputs(c, rows, nz, qscale)
    o, A = U.vatt_ref64(qkv, c)
    out = _call(qkv, c, ld_pad + 8)
    got = out[:nz, :rows, :c]
    ratio = U.vatt_within(got, o, A)
    print(f"vae attention bound C {c} rows {rows} nz {nz} qscale {qscale}: worst error / bound {ratio.max().item():.3f}")
    assert U.vatt_guards_untouched(out, rows, c)
    assert bool(torch.isfinite(got.float()).all())
    assert ratio.max().item() <= 1.0, ratio.max().item()
