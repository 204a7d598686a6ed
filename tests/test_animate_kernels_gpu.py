"""The three entries of include/vstyler_animate.h on the GPU against tests/animate_util.py.

vs_face_attn, exact tier: inputs on which every step but the final rounding is exact (animate_util.exact_problem)
-- the answer is known to the bit by integer logic.  Bound tier: random inputs against float64 attention over the
qn vs_head_rmsnorm produced on the device, every element within animate_util.face_attn_within's derived bound,
and the fused kernel equal to vs_head_rmsnorm followed by the kernel-order float32 restatement wherever that is
unambiguous.  vs_head_rmsnorm / vs_ln_silu: RowTally's bar (gpu_util).  The preconditions of the inputs and of
the bounds are held on the CPU by tests/test_animate_cpu.py."""
import pytest
import torch

import animate_util as A
import gpu_util as U

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
HD = A.HD


def run_face_attn(p, inplace, pad_o=0):
    """vs_face_attn on a problem dict -> (o [rows, H 128] on the CPU, the whole q buffer after the call, the
    whole o buffer).  Out of place the output rows carry pad_o sentinel columns."""
    from vstyler import kernels as K
    g = p["geom"]
    H = g["num_heads"]
    q = p["q"].cuda()
    k = p["k"].cuda().flatten(1, 2).flatten(2, 3)              # [B, frames N, H 128]
    v = p["v"].cuda().flatten(1, 2).flatten(2, 3)
    out = q if inplace else U.sentinel((q.shape[0], H * HD + pad_o))
    K.face_attn(q, k, v, p["wq"].cuda(), None if inplace else out, scale=p["scale"], **g)
    torch.cuda.synchronize()
    return out[:, :H * HD].cpu(), q.cpu(), out.cpu()


# ------------------------------------------------------------------------------------- vs_face_attn, exact
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("name", sorted(A.EXACT_CASES))
def test_face_attn_exact(name, inplace):
    p = A.exact_problem(name)
    H = p["geom"]["num_heads"]
    q0 = p["q"].clone()
    got, q_after, o_buf = run_face_attn(p, inplace, pad_o=8)
    same = (got.float() == p["ref"].float())                 # by value: -0 == +0
    assert bool(same.all()), (name, int((~same).sum()), got[~same][:4], p["ref"][~same][:4])
    if bool(p["pad"].any()):
        assert U.bit_zero(got[p["pad"]])
    # the columns outside the heads keep their bits; out of place q is not written at all
    assert U.same_bits(q_after[:, H * HD:], q0[:, H * HD:])
    if not inplace:
        assert U.same_bits(q_after, q0)
        assert U.untouched(o_buf[:, H * HD:])


def test_face_attn_shared_kv_and_strided_kv():
    """One K / V set for both samples (kv_bs 0), and K / V as the two column halves of one [.., 2 D] buffer
    (the model's linear1_kv output): the same bits as the plain layout."""
    from vstyler import kernels as K
    p = A.exact_problem("tpf6_f3_n5_h2_b2")
    g, H = p["geom"], p["geom"]["num_heads"]
    D = H * HD
    q = p["q"].cuda()
    k = p["k"].cuda().flatten(1, 2).flatten(2, 3)
    v = p["v"].cuda().flatten(1, 2).flatten(2, 3)
    wq = p["wq"].cuda()
    want = K.face_attn(q, k, v, wq, torch.empty_like(q), scale=p["scale"], **g)
    kv = torch.cat([k, v], dim=2).contiguous()
    got = K.face_attn(q, kv[:, :, :D], kv[:, :, D:], wq, torch.empty_like(q), scale=p["scale"], **g)
    assert U.same_bits(got[:, :D], want[:, :D])
    one = K.face_attn(q, k[:1], v[:1], wq, torch.empty_like(q), scale=p["scale"], **g)
    rpb = q.shape[0] // 2
    assert U.same_bits(one[:rpb, :D], want[:rpb, :D])
    two = K.face_attn(q[rpb:], k[:1], v[:1], wq, torch.empty_like(q[rpb:]), scale=p["scale"], **dict(g, batch=1))
    assert U.same_bits(one[rpb:, :D], two[:, :D])


# ------------------------------------------------------------------------------------- vs_face_attn, bound
@pytest.mark.parametrize("name", sorted(A.BOUND_CASES))
def test_face_attn_bound(name):
    from vstyler import kernels as K
    p = A.bound_inputs(name)
    g, H = p["geom"], p["geom"]["num_heads"]
    qn = K.head_rmsnorm(p["q"].cuda().clone(), p["wq"].cuda(), H).cpu()      # the device's own qn
    o64, Aa, smag = A.face_attn_ref64(qn, p["k"], p["v"], scale=p["scale"], **g)
    got, _, _ = run_face_attn(p, inplace=False)
    assert torch.isfinite(got.float()).all()
    ok, worst = A.face_attn_within(got, o64, Aa, smag, g["nkeys"])
    d = (got.double() - o64).abs()
    print(f"face_attn {name}: max |got - o| {d.max().item():.4g}, worst (d - bound) {worst:.4g}, "
          f"bit-identical to bf16(o64) {(got.float() == o64.to(BF16).float()).double().mean().item():.5f}")
    assert bool(ok.all()), (name, worst)
    # fused == vs_head_rmsnorm + the kernel-order float32 restatement wherever that is unambiguous
    amb = A.face_attn_ambiguous(o64, Aa)
    share = amb.double().mean().item()
    r32 = A.face_attn_order32(qn, p["k"], p["v"], scale=p["scale"], **g)
    diff = got.float() != r32.float()
    print(f"face_attn {name}: ambiguous share {share:.5f}, differing from the restatement {int(diff.sum())} "
          f"({int((diff & ~amb).sum())} unambiguous)")
    assert share <= A.FA_MAX_AMBIGUOUS
    assert not bool((diff & ~amb).any()), (name, int((diff & ~amb).sum()))
    # and in place on the device's qn route: norm in place, then attention by the unfused entries' own qn
    inpl, _, _ = run_face_attn(p, inplace=True)
    assert U.same_bits(inpl, got)


# --------------------------------------------------------------------------------------- vs_head_rmsnorm
def test_head_rmsnorm_rows():
    from vstyler import kernels as K
    tally = U.RowTally("head_rmsnorm")
    for rows, heads in A.ROW_SHAPES:
        for pad in (0, 16):
            g = torch.Generator().manual_seed(1000 * rows + heads + pad)
            x = (2.0 * torch.randn(rows, heads * HD, generator=g) + torch.randn(rows, 1, generator=g)).to(BF16)
            x[0, :HD] = 0                                                   # a zero head
            w = (1 + 0.1 * torch.randn(HD, generator=g)).to(BF16)
            buf = U.sentinel((rows, heads * HD + pad))
            buf[:, :heads * HD] = x.cuda()
            K.head_rmsnorm(buf, w.cuda(), heads)
            torch.cuda.synchronize()
            ref, bound = A.head_rmsnorm_ref(x, w, heads)
            tally.check(buf[:, :heads * HD], ref, bound, (rows, heads, pad))
            assert U.bit_zero(buf[0, :HD].cpu())
            assert U.untouched(buf[:, heads * HD:])
    tally.finish()


def test_head_rmsnorm_exact_pow2():
    """+-2^e rows: bf16(x rsqrt(4^e + eps)) is +-1 exactly, so the output is +-w to the bit."""
    from vstyler import kernels as K
    for rows, heads in A.ROW_SHAPES:
        x = A.exact_pow2_rows(rows * heads, HD, seed=rows + heads).view(rows, heads * HD)
        w = torch.pow(2.0, torch.arange(HD) % 3 - 1.0).to(BF16)
        got = K.head_rmsnorm(x.cuda().clone(), w.cuda(), heads).cpu()
        want = (torch.sign(x.float()).view(rows, heads, HD) * w.float()).view(rows, heads * HD).to(BF16)
        assert U.same_bits(got, want)


# -------------------------------------------------------------------------------------------- vs_ln_silu
def test_ln_silu_rows():
    from vstyler import kernels as K
    tally = U.RowTally("ln_silu")
    for dim in A.LN_SILU_DIMS:
        for rows in (1, 5):
            for pad, inplace in ((0, True), (8, False)):
                x, _, _, _ = U.row_inputs(rows, dim, seed=7 + rows)
                if rows > 1:
                    x[1] = 0                                                # a zero row stays zero
                src = U.sentinel((rows, dim + pad))
                src[:, :dim] = x.cuda()
                out = src if inplace else U.sentinel((rows, dim + 16))
                K.ln_silu(src[:, :dim], None if inplace else out[:, :dim])
                torch.cuda.synchronize()
                ref, bound, _ = A.ln_silu_ref(x)
                tally.check(out[:, :dim], ref, bound, (dim, rows, pad))
                if rows > 1:
                    assert U.bit_zero(out[1, :dim].cpu())
                assert U.untouched(out[:, dim:]) and U.untouched(src[:, dim:])
    tally.finish()


def test_ln_silu_exact_pow2():
    """+-2^e rows of an even split: mean 0 and variance 4^e exactly, so bf16(LN) = +-1 and the output is
    bf16(silu(+-1))."""
    from vstyler import kernels as K
    for dim in A.LN_SILU_DIMS:
        x = torch.ones(5, dim)
        x[:, dim // 2:] = -1
        x = (x * torch.pow(2.0, torch.arange(-2, 3).float()).view(5, 1)).to(BF16)
        got = K.ln_silu(x.cuda().clone()).cpu()
        want = A.silu64(torch.sign(x.float())).to(BF16)
        assert U.same_bits(got, want)


def test_ln_silu_every_bf16():
    """SiLU alone (norm = 0) over every finite bf16 value against float64, as vs_gelu_erf is held
    (test_i2v_kernels_gpu.py): within one bf16 ulp, and exact wherever the float64 value is not within 2 fp32
    ulps of a bf16 rounding midpoint."""
    from vstyler import kernels as K
    g = A.bf16_all_finite()
    n = g.numel() // 8 * 8
    g = g[:n]
    assert n > 65000
    ref64 = A.silu64(g)
    ref = ref64.to(BF16)
    amb = U.near_bf16_midpoint(ref64, 2)
    print(f"ln_silu (silu alone): ambiguous share {amb.double().mean().item():.6f} ({int(amb.sum())} of {n})")
    assert amb.double().mean().item() <= 0.01
    got = K.ln_silu(g.cuda().view(-1, 8).clone(), norm=False).cpu().view(-1)
    assert torch.isfinite(got.float()).all()
    dist = (U.bf16_ord(got) - U.bf16_ord(ref)).abs()
    bad = (dist > 0) & ~amb
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} non-ambiguous elements differ; first x {g[i].item()} got "
                             f"{got[i].item()} ref {ref64[i].item()}")
    assert int(dist.max()) <= 1, int(dist.max())


def test_unsupported_head_dim():
    f = 1 << 20
    assert U.call_rc("vs_head_rmsnorm", f, 512, 4, 8, 64, f, 1e-6, None) == 3
    assert U.call_rc("vs_face_attn", f, 512, f, f, 512, 0, f, 512, f, 1, 6, 8, 64, 1, 6, 5, 0, 1e-6, 0.1, None) == 3
