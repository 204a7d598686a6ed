"""vs_attn_fwd / vs_attn_fwd_add against float64 on every kernel route (gpu_util.ATTN_ROUTES: the default
-- attn_fwd_w4 from 4 key tiles, the optimistic 8-wave kernel below --, attn_impl=8, attn_nc=0,
attn_mfma=32), with the split-tail combine and the redo launch.

Exact tier: inputs (gpu_util.attn_exact_inputs, scale float32(ln 2)) on which every step of the
contract but the final bf16(acc * (1 / l)) is exact in fp32.  The bar per case: every element within
one bf16 ulp of the float64 -> fp32 -> bf16 reference, every element whose float64 value is not
within ATTN_WINDOW fp32 ulps of a bf16 rounding midpoint bit-identical, exact zeros +0.  A dropped
or doubled key, a padded-key count off by one or a piece merged with the wrong l moves most elements
by whole bf16 ulps.  The inputs' own preconditions (integer scores, exact sums, ambiguous share
<= 1 %, the redo rows' sides of 2^-4) are asserted without a GPU in test_kernel_refs_cpu.py.

Bound tier: random and spike inputs at the default scale, |got - o| <= 2^-8 (|o| + A) per element
(gpu_util.attn_within); the worst error / bound is printed per route and case.
"""
import pytest
import torch

import gpu_util as U

pytestmark = pytest.mark.gpu

CASES = U.attn_exact_cases()
_REFS = {}


@pytest.fixture(scope="module")
def K():
    from vstyler import kernels
    return kernels


@pytest.fixture(params=list(U.ATTN_ROUTES))
def route(request, opt):
    opt(**U.ATTN_ROUTES[request.param])
    return request.param


def exact_case(name, device="cpu"):
    """(q, k, v on the GPU; ref, ambiguous, ref64 dict on `device`; the case's arguments), computed once
    and never modified."""
    if name not in _REFS:
        c = CASES[name]
        q, k, v = (t.to(device) for t in U.attn_exact_inputs(**c))
        ref, amb, r = U.attn_exact_ref(q, k, v, c["H"], c["B"], c.get("shared_kv", False))
        share = U.attn_exact_preconditions(r, amb, smin=-14 if "r_rows" in c else -5)
        print(f"{name}: ambiguous share {share:.5f}")
        r = {n: (t.cpu() if isinstance(t, torch.Tensor) else t) for n, t in r.items()}
        _REFS[name] = (q.cuda(), k.cuda(), v.cuda(), ref.cpu(), amb.cpu(), r, c)
    return _REFS[name]


def meets_bar(got, ref, amb, r, what):
    ok, text = U.attn_exact_verdict(got, ref, amb, r["o"])
    print(f"{what}: {text}")
    if not ok:
        d = U.attn_midpoint_distance(got, ref, r["o"])
        print(f"{what}: distance of the differing elements from the midpoint, fp32 ulps: "
              f"min {d.min().item():.1f} max {d.max().item():.1f}")
    assert ok, (what, text)


def run(K, q, k, v, c, out=None):
    if out is None:
        out = U.sentinel((q.shape[0], c["H"] * 128))
    K.attention(q, k, v, out, c["H"], c["B"], scale=U.ATTN_EXACT_SCALE, shared_kv=c.get("shared_kv", False))
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------- exact tier
@pytest.mark.parametrize("Skv", U.ATTN_EDGE_SKV_W8 + U.ATTN_EDGE_SKV_W4)
def test_attention_exact_key_tile_edges(K, route, Skv):
    """(a) Sq 300 (a partial second q-block); Skv below 193 runs the 8-wave kernel on every route, from
    193 (4..8 key tiles, both parities of attn_fwd_w4's loop unrolled by two, every residue of the
    last tile near 0 / 31 / 32 / 33 / 63) attn_fwd_w4 by default."""
    q, k, v, ref, amb, r, c = exact_case(f"edge_skv{Skv}")
    meets_bar(run(K, q, k, v, c), ref, amb, r, f"{route} Skv {Skv}")


@pytest.mark.parametrize("Sq", U.ATTN_EDGE_SQ)
def test_attention_exact_query_edges(K, route, Sq):
    """(b) Skv 257; Sq around the 64-row wave of attn_fwd_w4 and the 32- / 16-row ones of the 8-wave
    kernel.  Output rows of stride H*128 + 8 with two extra rows: the pad columns and the extra rows
    keep their sentinel."""
    q, k, v, ref, amb, r, c = exact_case(f"edge_sq{Sq}")
    D, M = c["H"] * 128, c["B"] * Sq
    wide = U.sentinel((M + 2, D + 8))
    run(K, q, k, v, c, out=wide[:M, :D])
    meets_bar(wide[:M, :D], ref, amb, r, f"{route} Sq {Sq}")
    assert U.untouched(wide[:, D:]) and U.untouched(wide[M:])


def test_attention_exact_fused_qkv(K, route):
    """(c) q | k | v as column slices of one [B*S, 3*H*128] buffer."""
    q, k, v, ref, amb, r, c = exact_case("fused_qkv")
    D = c["H"] * 128
    qkv = torch.cat([q, k, v], dim=1)
    meets_bar(run(K, qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], c), ref, amb, r, f"{route} fused")


def test_attention_exact_shared_kv(K, route):
    """(c) one key set for both samples (batch strides 0)."""
    q, k, v, ref, amb, r, c = exact_case("shared_kv")
    assert k.shape[0] == c["Skv"]
    meets_bar(run(K, q, k, v, c), ref, amb, r, f"{route} shared_kv")


def test_attention_exact_redo_threshold(K, route):
    """(d) Skv 193 (63 padded keys subtracted from l by attn_fwd_w4).  Row 17 of every (sample, head) has
    r = -10: l ~ 0.09 >= 2^-4, its item stays on attn_fwd_w4; row 290 has r = -11: l ~ 0.044 < 2^-4, its
    item is redone by the checked kernel.  Both meet the bar; the item flags are zero afterwards."""
    from test_kernels_gpu import _flags_zero
    q, k, v, ref, amb, r, c = exact_case("redo")
    lrow = r["l"].view(c["B"], c["Sq"], c["H"])
    assert bool((lrow[:, 17] >= U.W4_LMIN).all()) and bool((lrow[:, 290] < U.W4_LMIN).all())
    meets_bar(run(K, q, k, v, c), ref, amb, r, f"{route} redo")
    assert _flags_zero(K)


def test_attention_exact_item_switch(K, route, opt):
    """(e) 288 items of 9 key tiles (8 keys in the last): several items per persistent block, with the
    XCD item queues and the static lists, and one item per block; every row against float64."""
    q, k, v, ref, amb, r, c = exact_case("switch", device="cuda")
    for queue, persist in ((1, 1), (0, 1), (1, 0), (0, 0)):
        opt(queue=queue, attn_persist=persist)
        meets_bar(run(K, q, k, v, c), ref, amb, r, f"{route} switch queue {queue} persist {persist}")


def test_attention_exact_split_tail(K, route, opt):
    """(f) 270 items on 256 CUs: the 14 tail items run as two pieces of 17 and 16 key tiles (the last
    tile 31 keys) merged by the combine kernel; with and without the split, every row against float64."""
    q, k, v, ref, amb, r, c = exact_case("split", device="cuda")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = K.attention_split_plan(c["B"], c["Sq"], c["Skv"], c["H"], cus)
    if cus == 256:
        assert plan == (256, 14, 2, 17), plan
    for split in (1, 0):
        opt(attn_split=split)
        meets_bar(run(K, q, k, v, c), ref, amb, r, f"{route} split {split}")


@pytest.mark.parametrize("Skv", [257, 449])
def test_attention_add_exact(K, route, Skv):
    """(g) vs_attn_fwd_add: o0 seeded integers in -4..4, o = bf16(o0 + bf16(attention)).  The fp32 sum is
    exact, so a non-ambiguous element has one answer and an ambiguous one two (gpu_util.attn_add_ref)."""
    q, k, v, ref, amb, r, c = exact_case(f"add_skv{Skv}")
    o0 = U.attn_add_o0(ref.shape, Skv)
    want, other = U.attn_add_ref(o0, ref, amb, r["o"])
    out = o0.cuda()
    K.attention_add(q, k, v, out, c["H"], c["B"], scale=U.ATTN_EXACT_SCALE)
    torch.cuda.synchronize()
    got = out.cpu()
    same = U.bits(got) == U.bits(want)
    either = same | (U.bits(got) == U.bits(other))
    print(f"{route} add Skv {Skv}: differing {int((~same).sum())} ({int((~either).sum())} outside both candidates) "
          f"of {got.numel()}, ambiguous {int(amb.sum())}")
    assert bool(either.all())


# ------------------------------------------------------------------------------------- bound tier
def random_case(name):
    if name not in _REFS:
        q, k, v, H, B = U.attn_bound_case(name)
        q, k, v = q.cuda(), k.cuda(), v.cuda()
        r = U.attn_ref64(q, k, v, H, B, 128 ** -0.5)
        assert bool(torch.isfinite(r["o"]).all()) and bool(torch.isfinite(r["A"]).all())
        _REFS[name] = (q, k, v, H, B, r)
    return _REFS[name]


@pytest.mark.parametrize("case", U.ATTN_BOUND_CASES)
def test_attention_within_derived_bound(K, route, case):
    """q ~ 2 N(0, 1), k, v ~ N(0, 1) (B x Sq x Skv x H) and the spike / low-row inputs of test_kernels_gpu's
    rescale tests, default scale: |got - o| <= 2^-8 (|o| + A) for every element."""
    q, k, v, H, B, r = random_case(case)
    out = U.sentinel((q.shape[0], H * 128))
    K.attention(q, k, v, out, H, B)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    worst = U.attn_within(out, r).max().item()
    print(f"route {route} case {case}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (route, case, worst)
