"""The CLIP image encoder on the GPU: WanImageEncoder.encode_image against tests/clip_util.py within the
oracle's floor (tiny towers at 257 and 17 tokens, two blocks at the real widths), width-80 attention through
the product route at the exact bar, the bit-identity checks (n = 2 == two n = 1 calls, a loaded file == the
directly built encoder), and the pipeline computing clip_feature itself."""
import pytest
import torch

import clip_util as C
import gpu_util as G
import i2v_util as I
from gpu_util import err

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SIZES = [(64, 96), (225, 223)]          # the two source sizes of the tower tests (n = 2 mixes them)


def within_floor(got, ref, ref64, tag):
    """The oracle-floor rule of tests/test_i2v_gpu.py: the floor is the restatement accumulating in float64
    against the float32 one."""
    fmx, frel = err(ref64, ref)
    mx, rel = err(got, ref)
    print(f"{tag}: max-abs {mx:.4g} rel-L2 {rel:.4g} (floor {fmx:.4g} / {frel:.4g})")
    assert rel <= 1.5 * frel + 2e-3 and mx <= 1.5 * fmx + 2e-2, (tag, mx, rel, fmx, frel)


def images(n, seed=60):
    return [C.sample_images(1, *SIZES[i % 2], seed + i)[0] for i in range(n)]


@pytest.fixture(scope="module")
def towers():
    """name -> (cfg, W, encoder, images, ref, ref64 of n = 2): weights, encoder and references once.

    The 17-token tower's seed.  The floor (float64 against float32 accumulation, both on the CPU) is a sparse
    cascade: an fp32 / fp64 difference of ~1e-7 flips a bf16 rounding on ~3e-5 of the elements per stage, and
    one flip re-rounds everything downstream to ~1e-3 relative.  With 17 x 320 elements per image the
    cascade may not start at all: over weight seeds 21..36 the floor's rel-L2 ranged from 0 (bit-identical) to
    2.4e-3, and differed between two CPUs for the same seed.  An implementation that follows vs_attn_fwd's
    contract (bf16 pre-scaled q, p rounded to bf16 before P V) is 2.4e-3 .. 2.8e-3 from the float32
    restatement whatever the floor (CPU emulation of the contract alone, seeds 21..24, both towers), which
    the rule's 1.5 floor + 2e-3 admits only when the floor is not degenerate.  Seed 26 is the first whose
    floor was above 5e-4 for n = 1 and n = 2 on both CPUs tried (1.6e-3 / 1.1e-3 and 1.4e-3): chosen from
    the restatements alone.  At 257 tokens the floor was 1.5e-3 .. 1.9e-3 for every seed."""
    out = {}
    for name, cfg, seed in (("tiny", C.TINY, 21), ("tiny17", C.TINY17, 26)):
        W = C.random_weights(cfg, seed=seed)
        ims = images(2)
        out[name] = (cfg, W, C.build(cfg, W), ims, C.encode_image(ims, W, cfg), C.encode_image64(ims, W, cfg))
    return out


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", ["tiny", "tiny17"])
def test_tiny_tower(towers, name, n):
    """dim 320 = 4 heads x 80, MLP 1280, 3 layers of which 2 run, at 257 tokens and at 17 (image_size 56)."""
    cfg, W, enc, ims, ref, ref64 = towers[name]
    got = enc.encode_image([u.cuda() for u in ims[:n]])
    assert got.shape == (n, C.tokens_of(cfg), cfg["dim"]) and got.dtype == BF16
    within_floor(got, ref[:n], ref64[:n], f"{name} n={n}")


def test_two_blocks_at_the_real_widths():
    """1280 / 16 heads / 5120, 257 tokens, seeded weights, two blocks."""
    cfg = C.REAL2
    W = C.random_weights(cfg, seed=22, extras=False)
    ims = images(1, seed=70)
    got = C.build(cfg, W).encode_image([ims[0].cuda()])
    within_floor(got, C.encode_image(ims, W, cfg), C.encode_image64(ims, W, cfg), "real widths, 2 blocks")


def test_attention_width_80_exact_through_the_product_route():
    """The exact problem at head width 80, s = 257, through vstyler.clip.attention_d80 (the route
    encode_image takes): every element within one bf16 ulp of the float64 -> bf16 answer, every
    non-ambiguous one bit-identical, exact zeros +0; the padded layout's 48 extra columns per head +0."""
    from vstyler.clip import attention_d80
    B, H, S = 2, 3, C.ATTN80_S
    q, k, v = C.attn80_exact_inputs(B, S, H, seed=7)
    ref, amb, r = C.attn80_exact_ref(q, k, v, H, B)
    G.attn_exact_preconditions(r, amb)
    qkv = torch.cat([C.pad_heads(t, H) for t in (q, k, v)], dim=1).cuda()
    out = G.sentinel((B * S + 1, H * 128))
    attention_d80(qkv, out[:B * S], H, B, scale=G.ATTN_EXACT_SCALE)
    val, pad = C.unpad_heads(out[:B * S].cpu(), H)
    ok, text = G.attn_exact_verdict(val, ref, amb, r["o"])
    print("width 80 exact, s = 257:", text)
    assert ok, text
    assert G.bit_zero(pad.contiguous()) and G.untouched(out[B * S:])


def test_attention_width_80_bound():
    """Random q ~ 2 N(0, 1), k, v ~ N(0, 1) at s in {77, 257}, scale 1/sqrt(80): |got - o| <= 2^-8 (|o| + A)."""
    from vstyler.clip import attention_d80
    B, H = 2, 3
    for S in (77, 257):
        q, k, v = C.attn80_random_inputs(B, S, H, seed=90 + S)
        r = C.attn80_ref64(q, k, v, H, B, 80 ** -0.5)
        qkv = torch.cat([C.pad_heads(t, H) for t in (q, k, v)], dim=1).cuda()
        out = G.sentinel((B * S, H * 128))
        attention_d80(qkv, out, H, B)
        val, pad = C.unpad_heads(out.cpu(), H)
        ratio = G.attn_within(val, r).max().item()
        print(f"width 80 random, s = {S}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0 and G.bit_zero(pad.contiguous())


def test_batch_of_two_equals_two_single_calls(towers):
    cfg, W, enc, ims, _, _ = towers["tiny"]
    both = enc.encode_image([u.cuda() for u in ims])
    one = [enc.encode_image([u.cuda()]) for u in ims]
    assert G.same_bits(both, torch.cat(one))
    # one [n, 3, H, W] tensor, and fp32 input (rounded to bf16 first), are the same call
    same = torch.stack([ims[0][0], ims[0][0]])
    assert G.same_bits(enc.encode_image(same.cuda()), torch.cat([one[0], one[0]]))
    assert G.same_bits(enc.encode_image([ims[1].float().cuda()]), one[1])


def test_load_models_builds_the_same_encoder(towers, tmp_path):
    from vstyler.clip import WanImageEncoder
    from vstyler.loader import load_models
    cfg, W, enc, ims, _, _ = towers["tiny17"]
    path = str(tmp_path / "models_clip_tiny.pth")
    torch.save({"model." + k: v for k, v in W.items()}, path)
    models = load_models([path], device="cuda")
    assert set(models) == {"wan_video_image_encoder"}
    loaded = models["wan_video_image_encoder"]
    assert isinstance(loaded, WanImageEncoder) and (loaded.image_size, loaded.num_layers) == (56, 3)
    x = [u.cuda() for u in ims]
    assert G.same_bits(loaded.encode_image(x), enc.encode_image(x))


@pytest.mark.parametrize("pos", [False, True], ids=["257", "514"])
def test_pipeline_computes_clip_feature(pos):
    """pipe(input_image=..., output_type="latents") on i2v_util's tiny I2V DiT (its img_emb takes 1280-wide
    features: a one-block 1280-wide encoder) equals the same call with clip_feature= passed explicitly."""
    from oracle import wan_vae_oracle as V
    from vae_util import TINY_VAE
    from vstyler import WanVideoPipeline, vae
    H, WD = 64, 96
    cfg = I.tiny_cfg(has_image_input=True, has_image_pos_emb=pos)
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit = I.build(cfg, I.random_weights(cfg, seed=5))
    pipe.vae = vae.WanVideoVAE(z_dim=16, dim=TINY_VAE["dim"], device="cuda").load_state_dict(
        V.random_vae_weights(TINY_VAE, seed=34))
    pipe.image_encoder = C.build(C.WIDE1, C.random_weights(C.WIDE1, seed=23, extras=False))
    _, _, _, cp, cn = I.inputs(cfg)
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (H, WD, 3), generator=g, dtype=torch.uint8)
    img2 = torch.randint(0, 256, (H, WD, 3), generator=g, dtype=torch.uint8)
    kw = dict(prompt_emb=cp, negative_prompt_emb=cn, input_image=img, end_image=img2, height=H, width=WD, num_frames=9,
              num_inference_steps=2, seed=3, tile_size=(4, 6), tile_stride=(2, 3), output_type="latents")
    got = pipe(**kw)
    frames = [pipe._image_frame(i, "image", H, WD)[:, :, 0] for i in (img, img2)]
    feats = [pipe.image_encoder.encode_image([f]) for f in frames]
    clip = torch.cat(feats, dim=1) if pos else feats[0]
    assert clip.shape == (1, 514 if pos else 257, 1280)
    assert G.same_bits(pipe.encode_clip_image(img, img2, H, WD), clip)
    want = pipe(clip_feature=clip, **kw)
    assert G.same_bits(got, want)
    other = pipe(clip_feature=torch.zeros_like(clip), **kw)
    assert not G.same_bits(got, other)
