"""CPU-side preconditions of the direct kernel-parity tests (no GPU): the references in gpu_util.py are
held to the assumptions the GPU tests rely on, on exactly the inputs those tests use, and the figures
are printed."""
import torch

from oracle import wan_oracle as O
import gpu_util as U


def test_t5_gelu_ambiguous_share():
    """At most 1 % of the every-bf16-pattern sweep may be excused as ambiguous (float64 tanh within 4 fp32
    ulps of a bf16 rounding midpoint); the reference chain itself is NaN exactly where g or a is."""
    a, g = U.t5_gelu_inputs()
    ref, amb = U.t5_gelu_mul_ref(a, g)
    share = amb.double().mean().item()
    print(f"t5_gelu_mul: ambiguous share {share:.6f} ({int(amb.sum())} of {amb.numel()})")
    assert share <= 0.01
    assert a.numel() % 256 != 0 and torch.unique(U.bits(g[:65536])).numel() == 65536
    assert not bool((amb & torch.isnan(ref)).any())


def test_near_bf16_midpoint_predicate():
    f = lambda bits_: torch.tensor([bits_], dtype=torch.int32).view(torch.float32).double()  # noqa: E731
    assert bool(U.near_bf16_midpoint(f(0x3F808000), 4))            # an exact midpoint
    assert bool(U.near_bf16_midpoint(f(0x3F808004), 4)) and bool(U.near_bf16_midpoint(f(0x3F807FFC), 4))
    assert not bool(U.near_bf16_midpoint(f(0x3F808005), 4)) and not bool(U.near_bf16_midpoint(f(0x3F807FFB), 4))
    assert not bool(U.near_bf16_midpoint(f(0x3F800000), 4)) and not bool(U.near_bf16_midpoint(f(0x3F810000), 4))
    assert not bool(U.near_bf16_midpoint(torch.zeros(1, dtype=torch.float64), 4))


def test_time_sinusoid_no_ambiguous_elements():
    t = U.sinusoid_inputs()
    assert t.numel() == 1051
    for dim in (2, 256):
        ref, amb = U.sinusoid_ref(dim, t)
        print(f"time_sinusoid dim {dim}: {int(amb.sum())} ambiguous of {amb.numel()}")
        assert ref.shape == (t.numel(), dim) and int(amb.sum()) == 0


def test_oracle_fp32_statistics_meet_the_row_bar():
    """The oracle's own fp32-statistics chains against the float64-statistics references, on the row
    tests' inputs: within the per-element bound and >= 99 % bit-identical for every dim -- the bar the
    kernels are held to is one a correct fp32 implementation meets."""
    for dim in U.ROW_LN_DIMS:
        tally_m, tally_a = U.RowTally(f"oracle fp32 LN+modulate dim {dim}"), U.RowTally(f"oracle fp32 LN affine dim {dim}")
        for rows in (1, 5):
            x, mod, w, b = U.row_inputs(rows, dim, seed=1)
            ref, bound = U.ln_modulate_ref(x, mod[:, 0], mod[:, 1])
            tally_m.check(O.modulate(O.layer_norm(x), mod[:, 0], mod[:, 1]), ref, bound)
            ref32, _ = U.ln_modulate_ref(x, mod[:, 0], mod[:, 1], dtype=torch.float32)
            tally_m.check(ref32, ref, bound)
            ref, bound = U.ln_affine_ref(x, w, b)
            tally_a.check(O.layer_norm(x, 1e-6, w, b), ref, bound)
        tally_m.finish()
        tally_a.finish()
    grid, off = (2, 3, 5), 13
    for dim in U.ROW_RMS_DIMS:
        tally = U.RowTally(f"oracle fp32 rmsnorm(+rope) dim {dim}")
        for rows in (1, 5):
            x, _, w, _ = U.row_inputs(rows, 3 * dim, seed=4)
            w = w[:dim].contiguous()
            freqs = O.rope_freqs(*grid)[off:off + rows]
            for i in range(2):
                xs = x[:, i * dim:(i + 1) * dim]
                ref, bound = U.rms_rope_ref(xs, w, 1e-6, freqs, dim // 128)
                got = O.rope_apply(O.rms_norm(xs, w).unsqueeze(0), freqs, dim // 128)[0]
                tally.check(got, ref, bound)
            ref, bound = U.rms_rope_ref(x[:, dim:2 * dim], w)
            tally.check(O.rms_norm(x[:, dim:2 * dim], w), ref, bound)
        tally.finish()


def test_t5_softmax_reference_is_the_oracle_expression():
    """gpu_util.t5_softmax_ref restates t5_attention's score path; an all-masked row is exactly uniform."""
    from oracle import t5_oracle as T
    L, nheads = 17, 4
    g = torch.Generator().manual_seed(0)
    emb = (0.5 * torch.randn(32, nheads, generator=g)).to(U.BF16)
    buckets = T.relative_position_bucket(L, L, 32)
    s = 2.0 * torch.randn(nheads, L, L, generator=g)
    v, p = U.t5_softmax_ref(s, emb, buckets, torch.zeros(L, dtype=torch.int32), 0, nheads)
    assert bool((v == torch.finfo(U.BF16).min).all()) and torch.equal(p, torch.full_like(p, 1.0 / L))
    mask = torch.ones(L, dtype=torch.int32)
    mask[5:] = 0
    v, p = U.t5_softmax_ref(s[1:3], emb, buckets, mask, 1, 2)
    assert bool((p[:, :, 5:] == 0).all()) and torch.allclose(p.sum(-1), torch.ones(2, L, dtype=torch.float64))
    want = s[1:3].to(U.BF16) + emb[buckets][..., 1:3].permute(2, 0, 1)
    assert torch.equal(v[:, :, :5], want[:, :, :5])
