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


# ------------------------------------------------------------------------------ VAE conv, exact problem
def test_conv_exact_preconditions_every_gpu_case():
    """Every case of test_vae_conv_exact_gpu.py, from the float64 reference alone: bf16(acc + bias) and
    bf16(that + res) are integers within +-256 (exact in bf16, every fp32 partial sum exact in any
    order), >= half of the outputs non-zero; the buffers have the guards the GPU test relies on (pad
    channels, a guard frame, the kept frames, NaN below t_lo and around the residual); the case list
    holds every value the halo kernel and each launcher must see."""
    cases = U.conv_exact_cases()
    for name, c in cases.items():
        p = U.conv_exact_problem(name)
        pre = U.conv_exact_preconditions(p)
        print(f"conv exact {name}: max |acc + bias| {pre['r1_max']:.0f}, + res {pre['r2_max']:.0f}, non-zero {pre['nonzero']:.3f}")
        want, written, x = p["want"], p["written"], p["x"]
        cout = c["split"] if c.get("split") else c["cout"]
        assert want.shape[-1] == p["ldy"] >= cout + 8 and p["ldy"] % (8 if U.conv_halo_eligible(c) == 3 else 4) == 0
        assert not bool(written[..., cout:].any()) and not bool(written[:, -1].any())
        assert all(not bool(written[:, f].any()) for f in c.get("keep", ()))
        assert bool(written[:, :c.get("y_t", c["out"][0]), :, :, :cout].any())
        assert U.untouched(want[~written]) and bool(torch.isfinite(want[written].float()).all())
        assert bool((want[written].double().abs() <= U.CONV_EXACT_LIMIT).all())
        t_lo = c.get("t_lo", 0)
        assert bool(torch.isnan(x[:, :t_lo].float()).all()) and bool(torch.isfinite(x[:, t_lo:].float()).all())
        assert set(x[:, t_lo:].double().unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert set(p["w"].double().unique().tolist()) <= {-1.0, 0.0, 1.0}
        if p["res"] is not None:
            assert U.untouched(p["res"][~written]) and int(p["res"][written].double().abs().max()) == 8
        assert x.numel() * 2 < 2 ** 20 * 4 and want.numel() * 2 < 2 ** 20 * 2        # a few hundred KB each
    # the k3 list: every value on each kernel it can reach
    k3 = {n: c for n, c in cases.items() if n.startswith("k3_") and "t_add" not in c}
    for nb, pairs in ((3, {(32, 96), (96, 192), (384, 96)}), (1, {(32, 16), (32, 3)}), (0, {(96, 64), (64, 128), (96, 100)})):
        sel = [c for c in k3.values() if U.conv_halo_eligible(c) == nb]
        assert {(c["cin"], c["cout"]) for c in sel} == pairs
        assert {c["t"] for c in sel} == {1, 4} and {c["res"] for c in sel} == {False, True}
        assert {c["hw"] for c in sel} == {(1, 1), (16, 32), (17, 33), (15, 31)}
        assert {c["t_lo"] for c in sel} == {0, 1, 2}
    for pair in ((96, 64), (64, 128), (96, 100)):
        assert {c["res"] for c in k3.values() if (c["cin"], c["cout"]) == pair} == {False, True}
    assert [cases[n]["cin"] // 32 for n in U.CONV_STEP_CASES] == list(range(1, 8))
    assert len(U.CONV_PIPELINES) == 6


def test_conv_exact_bar_has_teeth():
    """The reference against itself under the mistakes a gather can make: the first input column read as
    zero, frames below t_lo read, t_add ignored -- each changes the expected buffer (so the bitwise bar
    separates them), from the reference alone."""
    import torch.nn.functional as F
    p = U.conv_exact_problem("k3_96_192_15x31_t4_lo2_res")
    c = p["case"]
    x = p["x"].double().permute(0, 4, 1, 2, 3)
    w = p["w"].double()
    n_t = c["t"]

    def conv_of(xx, left):
        return F.conv3d(F.pad(xx, (left, 2 - left, 1, 1, 2, 0)), w)[:, :, :n_t]
    base = conv_of(torch.nan_to_num(x, nan=0.0), 1)
    live = p["want"][:, :n_t, :, :, :c["cout"]].double().permute(0, 4, 1, 2, 3)
    resid = p["res"][:, :n_t, :, :, :c["cout"]].double().permute(0, 4, 1, 2, 3)
    assert torch.equal(base + p["bias"].double().view(1, -1, 1, 1, 1) + resid, live)      # the restated reference
    col0 = torch.nan_to_num(x, nan=0.0)
    col0[..., 0] = 0                                                                     # xi >= 0 -> xi >= 1
    changed = (conv_of(col0, 1) != base)[:, :, c["t_lo"]:]
    assert changed[..., :2].double().mean().item() > 0.5 and not bool(changed[..., 2:].any())
    unmasked = conv_of(torch.nan_to_num(x, nan=1.0), 1)                                  # the t_lo predicate dropped
    assert bool((unmasked != base)[:, :, :c["t_lo"] + 2].any())
    q = U.conv_exact_problem("k3_32_96_17x33_t2_tadd")
    assert U.untouched(q["want"][:, 0]) and not U.untouched(q["want"][:, 1, :, :, :96])  # t_add ignored lands in frame 0


# ------------------------------------------------------------------------------ VAE attention references
def test_vae_attention_exact_preconditions_every_gpu_case():
    """Every (rows, C, g) of test_vae_attention_exact_gpu.py from the float64 scores alone: the gap to
    every non-tied key, times sc, >= 160; the tie counts are the group sizes; fl32(1 / g) >= 8 fp32 ulps
    from a bf16 midpoint; p * S exact in fp32."""
    worst = float("inf")
    sizes = set()
    for c in U.VATT_C:
        for rows in U.VATT_ROWS:
            for g in U.VATT_G:
                if g != "rows" and g >= rows:
                    continue
                qkv = U.vatt_exact_inputs(rows, c, g)
                ref, pre = U.vatt_exact_ref(qkv, c)
                U.vatt_exact_preconditions(pre, rows, g)
                assert bool(torch.isfinite(ref.float()).all())
                if rows > 1:
                    assert pre["nonzero"] > 0.5, (c, rows, g, pre)
                worst = min(worst, pre["min_gap"])
                sizes |= set(pre["sizes"])
        print(f"vae attention exact C {c}: smallest gap x sc so far {worst:.1f}")
    assert sizes >= {1, 2, 3, 5, 7, 32} | set(U.VATT_ROWS)
    # the closest any 1 / g comes to a bf16 midpoint, in fp32 ulps
    inv = 1.0 / torch.tensor(sorted(sizes), dtype=torch.float64)
    u = inv / torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.floor(torch.log2(inv)) - 23)
    dist = (torch.remainder(u, 65536.0) - 32768.0).abs()
    print(f"vae attention exact: group sizes {sorted(sizes)}, closest 1 / g to a bf16 midpoint: "
          f"1 / {sorted(sizes)[int(dist.argmin())]} at {dist.min().item():.0f} fp32 ulps")
    assert dist.min().item() >= U.VATT_WINDOW


def test_vae_attention_bars_are_met_by_fp32_and_have_teeth():
    """The two-pass kernel emulated in fp32 (bf16 P included) meets the exact bar on every exact case and
    the derived bound on every bound case; with the last key counted twice, one key dropped, or the V rows
    shifted by one it misses the exact bar on every shape of two rows or more (the g = rows case counts
    keys) and the bound on the cases named below."""
    muts = {"twice_last": dict(twice_last=True), "drop_key": dict(drop_key=0), "shift_v": dict(shift_v=True)}
    for c in U.VATT_C:
        for rows in U.VATT_ROWS:
            caught = {m: False for m in muts}
            for g in U.VATT_G:
                if g != "rows" and g >= rows:
                    continue
                qkv = U.vatt_exact_inputs(rows, c, g)
                ref, _ = U.vatt_exact_ref(qkv, c)
                assert U.same_bits(U.vatt_emulate_fp32(qkv, c), ref), (c, rows, g)
                for m, kw in muts.items():
                    if rows > 1 and not U.same_bits(U.vatt_emulate_fp32(qkv, c, **kw), ref):
                        caught[m] = True
                if g == "rows" and rows > 1:         # the key count itself
                    for m in ("twice_last", "drop_key"):
                        assert not U.same_bits(U.vatt_emulate_fp32(qkv, c, **muts[m]), ref), (c, rows, m)
            assert rows == 1 or all(caught.values()), (c, rows, caught)
    failed = {m: [] for m in muts}
    for c, rows, nz, ld_pad, qscale in U.VATT_BOUND_CASES:
        qkv = U.vatt_random_inputs(c, rows, nz, qscale)
        o, A = U.vatt_ref64(qkv, c)
        assert bool(torch.isfinite(o).all()) and bool((A >= o.abs() * (1 - 1e-12)).all())
        w = U.vatt_within(U.vatt_emulate_fp32(qkv, c), o, A).max().item()
        line = f"vae attention bound C {c} rows {rows} qscale {qscale}: fp32 emulation worst error / bound {w:.3f}"
        assert w <= 1.0, line
        for m, kw in muts.items():
            if rows > 1:
                wm = U.vatt_within(U.vatt_emulate_fp32(qkv, c, **kw), o, A).max().item()
                line += f", {m} {wm:.2f}"
                if wm > 1.0:
                    failed[m].append((c, rows, qscale))
        print(line)
    for m in muts:
        assert len(failed[m]) == sum(1 for case in U.VATT_BOUND_CASES if case[1] > 1), (m, failed[m])
