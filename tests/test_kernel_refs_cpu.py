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


# ------------------------------------------------------------------------------ attention references
def _exact(name):
    c = U.attn_exact_cases()[name]
    q, k, v = U.attn_exact_inputs(**c)
    ref, amb, r = U.attn_exact_ref(q, k, v, c["H"], c["B"], c.get("shared_kv", False))
    return c, q, k, v, ref, amb, r


def test_attention_exact_scale_leaves_q_unchanged():
    """At scale float32(ln 2) the kernels' c = fp32(scale) * log2(e) is within two fp32 ulps of 1 and
    bf16(fp32(q) * c) == q for EVERY finite bf16 q."""
    c = torch.tensor(U.ATTN_EXACT_SCALE, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    assert abs(c.item() - 1.0) <= 2 * 2.0 ** -23
    allbits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(U.BF16)
    fin = allbits[torch.isfinite(allbits.float())]
    assert U.same_bits(U.attn_prescale(fin, U.ATTN_EXACT_SCALE), fin)


def test_attention_exact_preconditions_every_gpu_case():
    """Every case of test_attention_exact_gpu.py, from the reference alone: integer scores in [-5, 2]
    ([-14, 2] with the redo rows), every sum exact in fp32 (max sum p |v| < 2^19), the pre-scaling a
    no-op, the ambiguous share <= 1 %, the expected exact zeros; the redo rows' l on their sides of 2^-4;
    vs_attn_fwd_add's fp32 sum exact.  (The two large cases are chunked over rows by attn_ref64.)"""
    worst = 0.0
    for name, c in U.attn_exact_cases().items():
        c, q, k, v, ref, amb, r = _exact(name)
        share = U.attn_exact_preconditions(r, amb, smin=-14 if "r_rows" in c else -5)
        worst = max(worst, share)
        zeros = int((r["o"] == 0).sum())
        print(f"attention exact {name}: ambiguous share {share:.5f} ({int(amb.sum())} of {amb.numel()}), exact zeros {zeros}")
        assert (zeros > 0) == (c["Skv"] < 8) and U.bit_zero(ref[r["o"] == 0])
        assert bool((ref.float() >= 0).all()) and bool(torch.isfinite(ref.float()).all())
        if "r_rows" in c:
            lrow = r["l"].view(c["B"], c["Sq"], c["H"])
            other = torch.ones(c["Sq"], dtype=torch.bool)
            other[[17, 290]] = False
            assert bool((lrow[:, 17] >= U.W4_LMIN).all()) and bool((lrow[:, 290] < U.W4_LMIN).all())
            assert bool((lrow[:, other] >= 1.0).all())
            print(f"attention exact {name}: l of the r = -10 rows {lrow[:, 17].min():.4f}..{lrow[:, 17].max():.4f}, "
                  f"of the r = -11 rows {lrow[:, 290].min():.4f}..{lrow[:, 290].max():.4f}")
        elif name not in ("edge_skv1",):
            assert r["l"].min().item() >= U.W4_LMIN
        if name.startswith("add_"):
            o0 = U.attn_add_o0(ref.shape, c["Skv"])
            want, other = U.attn_add_ref(o0, ref, amb, r["o"])
            assert bool((U.bits(other) == U.bits(want))[~amb].all()) and int(o0.min()) == -4 and int(o0.max()) == 4
            assert torch.equal(want.double(), (o0.double() + ref.double()).float().to(U.BF16).double())
    print(f"attention exact: worst ambiguous share {worst:.5f}")


def test_attention_exact_bar_is_met_by_fp32_and_has_teeth():
    """The contract in fp32 on the CPU meets the exact bar on every key-tile-edge case; with the last key
    dropped, or 1 added to l, it misses it (from 31 keys on: more than a quarter of the non-ambiguous
    elements flip)."""
    for skv in U.ATTN_EDGE_SKV_W8 + U.ATTN_EDGE_SKV_W4:
        c, q, k, v, ref, amb, r = _exact(f"edge_skv{skv}")
        args = (q, k, v, c["H"], c["B"], U.ATTN_EXACT_SCALE)
        ok, text = U.attn_exact_verdict(U.attn_emulate_fp32(*args), ref, amb, r["o"])
        assert ok, (skv, text)
        if skv < 31:
            continue
        for mut in (dict(drop_last_key=True), dict(l_add=1.0)):
            got = U.attn_emulate_fp32(*args, **mut)
            ok, text = U.attn_exact_verdict(got, ref, amb, r["o"])
            flipped = ((U.bits(got) != U.bits(ref)) & ~amb).double().mean().item()
            print(f"attention exact Skv {skv} {mut}: {flipped:.3f} of the elements flip")
            assert not ok and flipped > 0.25, (skv, mut, flipped)


def test_attention_bound_is_met_by_fp32():
    """|got - o| <= 2^-8 (|o| + A): the contract in fp32 on the CPU stays within it on the random shapes
    (the optimistic form cannot run the spike cases; their references are checked to be finite).  The
    figure with P packed by truncation is printed only: with l summed from the same truncated p its
    bias of half a bf16 ulp cancels in the ratio, so this bound does not separate it from rounding."""
    for name in ["x".join(map(str, s)) for s in U.ATTN_RANDOM_SHAPES]:
        q, k, v, H, B = U.attn_bound_case(name)
        r = U.attn_ref64(q, k, v, H, B, 128 ** -0.5)
        assert bool(torch.isfinite(r["o"]).all()) and bool((r["A"] >= r["o"].abs() * (1 - 1e-12)).all())
        w = U.attn_within(U.attn_emulate_fp32(q, k, v, H, B, 128 ** -0.5), r).max().item()
        wt = U.attn_within(U.attn_emulate_fp32(q, k, v, H, B, 128 ** -0.5, truncate_p=True), r).max().item()
        print(f"attention bound {name}: fp32 emulation worst error / bound {w:.3f}, truncated P {wt:.3f}")
        assert w <= 1.0, (name, w)
    for name in U.ATTN_SPIKE_KINDS:
        q, k, v, H, B = U.attn_bound_case(name)
        r = U.attn_ref64(q, k, v, H, B, 128 ** -0.5)
        assert bool(torch.isfinite(r["o"]).all()) and bool(torch.isfinite(r["A"]).all())
