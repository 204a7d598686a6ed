"""Wan2.2-Animate without a GPU: the restatements of tests/animate_util.py against the reference's own float64
output (tests/golden/animate_ref.npz), the checkpoint split and its hashes, the inpaint form of y against a
literal restatement of the reference's unit, the argument errors, and the preconditions of the kernel tests'
exact inputs and bounds (an fp32 CPU emulation of vs_face_attn's contract stays inside the bar, five wrong
variants of it leave it)."""
import json
import os

import numpy as np
import pytest
import torch

import animate_util as A
import gpu_util as U
import i2v_util as I

BF16 = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------- the fixture
def _fixture_inputs():
    g = torch.Generator().manual_seed(31)
    motion = torch.randn((1, 9, 32), generator=g).to(BF16).double()
    x = torch.randn((1, 24, 256), generator=g).to(BF16).double()
    return motion, x


def test_restatements_equal_the_reference_fixture():
    fx = np.load(os.path.join(HERE, "golden", "animate_ref.npz"))
    W = A.adapter_weights(256, 2, 6, in_dim=32, seed=int(fx["seed"]))
    for k in ("face_encoder.conv1_local.conv.weight", "face_adapter.fuser_blocks.0.linear1_kv.weight",
              "face_adapter.fuser_blocks.0.q_norm.weight"):
        assert abs(W[k].double().abs().sum().item() - float(fx["abs_sum." + k])) < 1e-9, f"seeded weights drifted: {k}"
    motion, x = _fixture_inputs()
    tok = A.pure_float64(lambda: A.face_encoder(motion, W))
    want = torch.from_numpy(fx["face_encoder"])
    assert tok.shape == want.shape == (1, 3, 5, 256)
    assert (tok - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    mv = torch.cat([torch.zeros_like(want[:, :1]), want], dim=1)
    res = A.pure_float64(lambda: A.face_block(x, mv, W, "face_adapter.fuser_blocks.0.", 2))
    want = torch.from_numpy(fx["face_block"])
    assert res.shape == want.shape == (1, 24, 256)
    assert (res - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    # with the rounding points on, the restatement stays a bf16-rounding distance from it
    rounded = A.face_block(x.to(BF16), mv.to(BF16), W, "face_adapter.fuser_blocks.0.", 2)
    assert rounded.dtype == BF16 and U.err(rounded, want)[1] < 2e-2


# --------------------------------------------------------------------------------------------- the loader
def test_animate_14b_key_set_hashes_and_splits():
    from vstyler import loader as L
    from vstyler.models import WanAnimateAdapter, WanModel
    with open(os.path.join(HERE, "golden", "animate_keys.json")) as f:
        keys = json.load(f)
    assert len(keys) == 138
    i2v = "6bfcfb3b342cb286ce886889d519a77e"
    dit = WanModel(device="meta", **dict(L.WAN_COMMON, **L.WAN_I2V_DIT_CONFIGS[i2v]))
    sd = dict(dit.state_dict())
    assert L.hash_state_dict_keys(sd) == i2v
    sd.update({k: torch.empty(s, device="meta") for k, s in keys.items()})
    assert L.hash_state_dict_keys(sd) == L.WAN_ANIMATE_HASH == "31fa352acb8a1b1d33cd8764273d80a2"
    rest, ad = L.split_animate(sd)
    assert L.hash_state_dict_keys(rest) == i2v and set(ad) == set(keys)
    mine = {k: list(v.shape) for k, v in WanAnimateAdapter(device="meta").state_dict().items()}
    assert mine == {k: s for k, s in keys.items() if not k.startswith("motion_encoder.")}
    assert L.split_animate(rest) == (rest, {})


def test_load_models_splits_a_tiny_animate_file(tmp_path):
    from vstyler.loader import load_models
    from vstyler.models import WanAnimateAdapter, WanModel
    cfg = A.tiny_cfg()
    W = I.random_weights(cfg, seed=5)
    Wa = A.adapter_weights(cfg["dim"], cfg["num_heads"], cfg["num_layers"], in_dim=32)
    me = {"motion_encoder.dec.direction.weight": torch.randn(512, 20), "motion_encoder.enc.fc.0.bias": torch.randn(512)}
    path = str(tmp_path / "animate_tiny.pth")
    torch.save({**W, **Wa, **me}, path)
    models = load_models([path], device="cpu")
    assert set(models) == {"wan_video_dit", "wan_video_animate_adapter"}
    dit, ad = models["wan_video_dit"], models["wan_video_animate_adapter"]
    assert isinstance(dit, WanModel) and isinstance(ad, WanAnimateAdapter)
    assert (dit.dim, dit.in_dim, len(dit.blocks), dit.has_image_input) == (256, 36, 6, True)
    assert (ad.dim, ad.num_heads, ad.num_layers, ad.face_encoder.in_dim) == (256, 2, 6, 32)
    assert len(ad.face_adapter.fuser_blocks) == 2
    got = ad.state_dict()
    assert set(got) == set(Wa) and all(torch.equal(got[k], Wa[k]) for k in Wa)
    assert set(ad.motion_encoder) == set(me) and all(torch.equal(ad.motion_encoder[k], me[k]) for k in me)
    assert ad.motion_encoder["motion_encoder.enc.fc.0.bias"].dtype == torch.float32          # unconverted
    # an adapter that does not fit its DiT
    bad = {k: v for k, v in Wa.items() if ".fuser_blocks.1." not in k}
    torch.save({**W, **bad}, path)
    with pytest.raises(ValueError, match="fuser blocks"):
        load_models([path], device="cpu")
    # quantize_fp8_ converts DiT blocks only: the adapter has none
    from vstyler.models import DiTBlock
    assert not [m for m in ad.modules() if isinstance(m, DiTBlock)]
    import diffsynth.models.wan_video_animate_adapter as drop_in
    assert drop_in.WanAnimateAdapter is WanAnimateAdapter


# ----------------------------------------------------------------------------------------- the inpaint y
def test_inpaint_y_and_mask_layout_against_the_literal_unit():
    from vstyler.pipeline import animate_i2v_mask, animate_inpaint_y
    g = torch.Generator().manual_seed(9)
    F_, Hh, Ww, h, w = 5, 32, 48, 4, 6
    ref = torch.randn((1, 16, 1, h, w), generator=g).to(BF16)
    bg = torch.randn((1, 16, 2, h, w), generator=g).to(BF16)
    m8 = torch.randint(0, 256, (F_, Hh, Ww), generator=g, dtype=torch.uint8)
    m8[:, :8] = 255
    m8[:, 8:16] = 0
    pre = (m8.to(BF16) * (1.0 / 255) + 0)[None, None]                    # preprocess_video(max_value=1, min_value=0)
    want = A.inpaint_y(ref[0], bg[0], pre)
    mask = (1 - (m8.float() * (1.0 / 255)).to(BF16).float()).to(BF16)
    got = animate_inpaint_y(ref, bg, mask)
    assert got.shape == want.shape == (1, 20, 3, h, w) and got.dtype == BF16
    assert U.same_bits(got, want)
    assert bool((got[0, :4, 0] == 1).all())                               # y_ref: mask 1
    # the first mask frame four times, then groups of four: latent frame 1 channel c is pixel frame 1 + c
    lay = animate_i2v_mask(torch.arange(5.0).view(5, 1, 1).expand(5, Hh, Ww), h, w)
    assert lay.shape == (4, 2, h, w)
    assert lay[:, 0, 0, 0].tolist() == [0, 0, 0, 0] and lay[:, 1, 0, 0].tolist() == [1, 2, 3, 4]
    assert torch.equal(lay, A.get_i2v_mask(2, h, w, 0, torch.arange(5.0).view(1, 5, 1, 1).expand(1, 5, h, w)))
    with pytest.raises(ValueError, match="4 k \\+ 1"):
        animate_i2v_mask(torch.zeros(4, Hh, Ww), h, w)


# ------------------------------------------------------------------------------------- argument errors
@pytest.fixture(scope="module")
def cpu_models():
    cfg = A.tiny_cfg()
    from vstyler.models import WanAnimateAdapter, WanModel
    dit = WanModel(dim=256, in_dim=36, ffn_dim=cfg["ffn_dim"], out_dim=16, text_dim=4096, freq_dim=256, eps=1e-6,
                   patch_size=(1, 2, 2), num_heads=2, num_layers=6, has_image_input=True, device="meta")
    ad = WanAnimateAdapter(dim=256, num_heads=2, num_layers=6, in_dim=32, device="meta")
    return dit, ad


def test_model_fn_argument_errors(cpu_models):
    from vstyler import model_fn_wan_video
    from vstyler.models import WanAnimateAdapter
    dit, ad = cpu_models
    lat = torch.zeros(1, 16, 3, 8, 12)
    pose = torch.zeros(1, 16, 2, 8, 12)
    motion = torch.zeros(1, 5, 32)
    base = dict(latents=lat, timestep=torch.tensor([500.0]), context=torch.zeros(1, 8, 4096), y=torch.zeros(1, 20, 3, 8, 12),
                clip_feature=torch.zeros(1, 257, 1280))
    with pytest.raises(ValueError, match="animate_adapter"):
        model_fn_wan_video(dit, pose_latents=pose, **base)
    with pytest.raises(ValueError, match="do not match the DiT"):
        model_fn_wan_video(dit, animate_adapter=WanAnimateAdapter(dim=256, num_heads=2, num_layers=11, device="meta"),
                           animate_face_motion=motion, **base)
    with pytest.raises(NotImplementedError, match="animate_face_motion="):
        model_fn_wan_video(dit, animate_adapter=ad, face_pixel_values=torch.zeros(1, 3, 5, 512, 512), **base)
    cases = {"sliding window": dict(sliding_window_size=2, sliding_window_stride=1), "tea_cache": dict(tea_cache=object()),
             "VACE": dict(vace=object(), vace_context=torch.zeros(1, 96, 3, 8, 12)),
             "reference_latents": dict(reference_latents=torch.zeros(1, 16, 1, 8, 12)),
             "first_frame_latents": dict(fuse_vae_embedding_in_latents=True),
             "camera control": dict(camera_tokens=torch.zeros(72, 256)), "slg_blocks": dict(slg_blocks=(1,))}
    for what, kw in cases.items():
        for inputs in (dict(pose_latents=pose), dict(animate_face_motion=motion)):
            with pytest.raises(NotImplementedError, match=what):
                model_fn_wan_video(dit, animate_adapter=ad, **inputs, **kw, **base)


def test_pipeline_argument_errors(cpu_models):
    from vstyler import WanVideoPipeline
    from vstyler.pipeline import animate_face_motion_batch
    dit, ad = cpu_models
    pipe = WanVideoPipeline(device="cpu")
    pipe.dit = dit
    img = torch.zeros(32, 48, 3, dtype=torch.uint8)
    call = dict(prompt_emb=torch.zeros(1, 8, 4096), negative_prompt_emb=torch.zeros(1, 8, 4096), height=32, width=48,
                num_frames=9, output_type="latents", clip_feature=torch.zeros(1, 257, 1280))
    with pytest.raises(NotImplementedError, match="animate_face_motion="):
        pipe(animate_face_video=[img] * 5, input_image=img, **call)
    with pytest.raises(ValueError, match="animate_adapter"):
        pipe(pose_latents=torch.zeros(1, 16, 2, 4, 6), input_image=img, **call)
    pipe.animate_adapter = ad
    with pytest.raises(ValueError, match="input_image"):
        pipe(pose_latents=torch.zeros(1, 16, 2, 4, 6), **call)
    with pytest.raises(ValueError, match="go together"):
        pipe(animate_inpaint_video=[img] * 5, input_image=img, **call)
    lat = torch.zeros(1, 16, 3, 4, 6)
    ctx = torch.zeros(1, 8, 4096)
    pose, motion = torch.zeros(1, 16, 2, 4, 6), torch.zeros(1, 5, 32)
    den = dict(num_inference_steps=2, y=torch.zeros(1, 20, 3, 4, 6), clip_feature=torch.zeros(1, 257, 1280))
    cases = {"sliding window": dict(sliding_window_size=2, sliding_window_stride=1), "tea_cache": dict(tea_cache=object()),
             "reference_latents": dict(reference_latents=torch.zeros(1, 16, 1, 4, 6)),
             "first_frame_latents": dict(first_frame_latents=torch.zeros(1, 16, 1, 4, 6))}
    for what, kw in cases.items():
        with pytest.raises(NotImplementedError, match=what):
            pipe.denoise(lat, ctx, ctx, pose_latents=pose, animate_face_motion=motion, **den, **kw)
    pipe.vace = object()
    with pytest.raises(NotImplementedError, match="VACE"):
        pipe.denoise(lat, ctx, ctx, pose_latents=pose, vace_context=torch.zeros(1, 96, 3, 4, 6), **den)
    pipe.vace, pipe.dit2 = None, dit
    with pytest.raises(NotImplementedError, match="dit2"):
        pipe.denoise(lat, ctx, ctx, animate_face_motion=motion, **den)
    pipe.dit2 = None
    with pytest.raises(NotImplementedError, match="UniPC"):
        pipe.denoise_unipc(lat, ctx, ctx, pose_latents=pose)
    with pytest.raises(NotImplementedError, match="UniPC"):
        pipe.denoise_unipc(lat, ctx, ctx, animate_face_motion=motion)
    # the unconditioned sample's motion: required with CFG, one vector or a full sequence
    with pytest.raises(ValueError, match="animate_face_motion_uncond"):
        animate_face_motion_batch(motion, None, True)
    assert animate_face_motion_batch(motion[0], None, False).shape == (1, 5, 32)
    one = torch.arange(32.0)
    both = animate_face_motion_batch(motion, one, True)
    assert both.shape == (2, 5, 32) and torch.equal(both[1], one.expand(5, 32))
    full = torch.randn(5, 32)
    assert torch.equal(animate_face_motion_batch(motion, full, True)[1], full)
    assert torch.equal(animate_face_motion_batch(motion, one[None], True), both)
    with pytest.raises(ValueError, match="animate_face_motion_uncond"):
        animate_face_motion_batch(motion, torch.zeros(3, 32), True)


# ------------------------------------------------------------------ the kernel tests' preconditions and bar
@pytest.mark.parametrize("name", sorted(A.EXACT_CASES))
def test_exact_inputs_preconditions_and_emulation(name):
    p = A.exact_problem(name)
    A.exact_preconditions(p)
    got = A.emulate(p)
    assert torch.equal(got.float(), p["ref"].float()), name          # the fp32 emulation of the contract: to the bit


def test_exact_cases_cover_the_edges():
    cases = list(A.EXACT_CASES.values())
    assert {c[4] for c in cases} >= {1, 6, 63, 65} and {c[3] for c in cases} >= {1, 3}
    assert {c[5] for c in cases} >= {1, 2, 4, 5, 8} and {c[2] for c in cases} >= {1, 2, 12, 40}
    ties = set()
    for name in A.EXACT_CASES:
        p = A.exact_problem(name)
        ties |= {(p["geom"]["nkeys"], int(t)) for t in p["tie_sizes"]}
    assert ties >= {(1, 1), (2, 1), (2, 2), (4, 1), (4, 4), (8, 1), (8, 8), (5, 2), (8, 4)}, sorted(ties)
    b, rpb, _, frames, tpf, _, off, _, _ = A.EXACT_CASES["offset_crosses_frame"]
    assert off % tpf and off // tpf != (off + rpb - 1) // tpf and (off + rpb) <= frames * tpf and b == 2
    assert A.exact_problem("pad_rows")["pad"].sum() == 44 and A.EXACT_CASES["tpf65_f3_n5_h40_b2_ld"][8] > 0


def _bound_problem(name):
    p = A.bound_inputs(name)
    H = p["geom"]["num_heads"]
    qn = A.head_rmsnorm_order32(p["q"], p["wq"], H)
    return p, qn, A.face_attn_ref64(qn, p["k"], p["v"], scale=p["scale"], **p["geom"])


@pytest.mark.parametrize("name", sorted(A.BOUND_CASES))
def test_bound_tier_emulation_inside_and_ambiguity_cap(name):
    p, qn, (o64, Aa, smag) = _bound_problem(name)
    got = A.face_attn_order32(qn, p["k"], p["v"], scale=p["scale"], **p["geom"])
    ok, worst = A.face_attn_within(got, o64, Aa, smag, p["geom"]["nkeys"])
    assert bool(ok.all()), (name, worst)
    # the rounding term is half a bf16 ulp of the rounded value, not a flat 2^-9 |o|: the float64 answer itself,
    # correctly rounded to bf16, is further than 2^-9 |o| from it on some elements (bf16 keeps 8 significant
    # bits: half an ulp is between 2^-9 |x| and 2^-8 |x|), and never further than the half ulp
    ideal = o64.to(BF16).double()
    if p["geom"]["nkeys"] > 1:
        assert bool(((ideal - o64).abs() > 2.0 ** -9 * o64.abs()).any())
    half_ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.floor(torch.log2(o64.abs().clamp(min=1e-30))) - 8)
    # (torch rounds float64 -> fp32 -> bf16: the two roundings can exceed the half ulp by 2^-16 of it)
    assert bool(((ideal - o64).abs() <= half_ulp * (1 + 2.0 ** -14))[o64 != 0].all())
    share = A.face_attn_ambiguous(o64, Aa).double().mean().item()
    assert share <= A.FA_MAX_AMBIGUOUS, (name, share)


@pytest.mark.parametrize("mutation", sorted(A.MUTATIONS))
def test_every_mutation_leaves_the_bar(mutation):
    """Each wrong variant of the contract fails the exact tier or the bound tier on at least one case (and the
    cases it is built to fail are named): the bar can tell them from the contract."""
    kw = A.MUTATIONS[mutation]
    failed = []
    for name in A.EXACT_CASES:
        p = A.exact_problem(name)
        got = torch.nan_to_num(A.emulate(p, **kw).float(), nan=1e9)
        if not torch.equal(got, p["ref"].float()):
            failed.append(name)
    for name in A.BOUND_CASES:
        p, qn, (o64, Aa, smag) = _bound_problem(name)
        got = torch.nan_to_num(A.emulate(p, **kw).float(), nan=1e9)
        if not bool(A.face_attn_within(got, o64, Aa, smag, p["geom"]["nkeys"])[0].all()):
            failed.append(name)
    must = {"eps dropped": "b2_tpf65_f3_n5_h12", "wq not applied": "tpf6_f3_n5_h2_b2",
            "last key dropped": "tpf65_f3_n5_h40_b2_ld", "frame index off by one at a frame edge": "tpf63_f3_n8_h12",
            "K/V of the wrong CFG sample": "offset_crosses_frame"}[mutation]
    assert must in failed, (mutation, failed)


def test_row_references_preconditions():
    """+-2^e rows: the per-head RMSNorm reference gives +-w to the bit; the LayerNorm -> SiLU reference of an
    even +-2^e split gives bf16(silu(+-1)); a zero row stays zero; SiLU's ambiguous share over every bf16 value
    is under 1 %."""
    x = A.exact_pow2_rows(6, 128, seed=2)
    w = torch.pow(2.0, torch.arange(128) % 3 - 1.0).to(BF16)
    ref, bound = A.head_rmsnorm_ref(x, w, 1)
    assert torch.equal(ref.float(), torch.sign(x.float()) * w.float())
    assert U.same_bits(A.head_rmsnorm_order32(x, w, 1), ref)
    xs = torch.ones(5, 8)
    xs[:, 4:] = -1
    xs = (xs * torch.pow(2.0, torch.arange(-2, 3).float()).view(5, 1)).to(BF16)
    ref, _, _ = A.ln_silu_ref(xs)
    assert U.same_bits(ref, A.silu64(torch.sign(xs.float())).to(BF16))
    z, _, _ = A.ln_silu_ref(torch.zeros(2, 1024, dtype=BF16))
    assert U.bit_zero(z)
    g = A.bf16_all_finite()
    assert U.near_bf16_midpoint(A.silu64(g), 2).double().mean().item() <= 0.01
