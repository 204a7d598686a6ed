"""The CLIP image encoder without a GPU: the loader's recognition and config, what load_state_dict keeps
and drops, the pipeline's flow around pipe.image_encoder (a stub that records its calls), the
preprocessing restatement against torch's own CPU fp32 path, and the preconditions of the interval test
and of the width-80 exact attention inputs, asserted from the references alone."""
import pytest
import torch
import torch.nn.functional as F

import clip_util as C
import gpu_util as G

BF16 = torch.bfloat16


# --------------------------------------------------------------------------------------------- loader
def _meta(cfg, prefix):
    return {prefix + k: torch.empty(s, dtype=BF16, device="meta") for k, s in C.param_shapes(cfg).items()}


@pytest.mark.parametrize("prefix", ["", "model."])
@pytest.mark.parametrize("cfg", [C.TINY, C.TINY17, C.REAL2], ids=["tiny", "tiny17", "real2"])
def test_config_from_a_meta_state_dict(cfg, prefix):
    """Recognition by the visual tower's keys, the config read off the shapes alone (no tensor data)."""
    from vstyler.clip import config_from_shapes
    sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in _meta(cfg, prefix).items()}
    assert config_from_shapes(sd) == cfg
    assert config_from_shapes({k: v for k, v in sd.items() if "to_qkv" not in k}) is None


def test_reference_hash_and_model_id_are_listed():
    from vstyler import loader, pipeline
    assert loader.CLIP_HASH == "5941c53e207d62f20f9025686193c40b"
    assert "models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth" in open(pipeline.__file__).read()


@pytest.mark.parametrize("prefix", ["", "model."])
def test_build_image_encoder_keeps_and_drops(prefix):
    from vstyler.clip import WanImageEncoder
    from vstyler.loader import build_dit, build_image_encoder, build_text_encoder, build_vae
    cfg = C.TINY17
    W = C.random_weights(cfg, prefix=prefix)
    enc = build_image_encoder(W, "cpu")
    assert isinstance(enc, WanImageEncoder)
    assert (enc.dim, enc.num_heads, enc.mlp_ratio, enc.num_layers, enc.image_size, enc.tokens) == (320, 4, 4, 3, 56, 17)
    assert build_dit(W, "cpu") is None and build_vae(W, "cpu") is None and build_text_encoder(W, "cpu") is None
    assert build_image_encoder({"blocks.0.attn.q.weight": torch.zeros(4, 4)}, "cpu") is None
    # nothing of the last block, post_norm, head, log_scale or the text tower is held
    names = set(enc.w)
    assert not any(n.startswith("2.") or "post_norm" in n or "head" in n or "textual" in n or "log_scale" in n
                   for n in names), sorted(names)
    assert {n.split(".")[0] for n in names if n[0].isdigit()} == {"0", "1"}
    held = sum(t.numel() for t in enc.w.values())
    d, H = cfg["dim"], cfg["num_heads"]
    per_block = 4 * d + (3 * H * 128) * (d + 1) + d * H * 128 + d + 2 * (4 * d * d) + 4 * d + d
    assert held == d * 640 + d + 16 * d + 2 * d + 2 * per_block
    # patch weight [dim, 640]: the conv weight in (c, ky, kx) order, columns 588.. zero
    pw = enc.w["patch"]
    assert pw.shape == (d, 640) and pw.dtype == BF16
    assert torch.equal(pw[:, :588], W[prefix + "visual.patch_embedding.weight"].reshape(d, 588))
    assert G.bit_zero(pw[:, 588:])
    # row0 = bf16(bf16(cls) + pos[0]); pos[1:] apart
    cls, pos = W[prefix + "visual.cls_embedding"], W[prefix + "visual.pos_embedding"]
    assert torch.equal(enc.w["row0"], (cls[0, 0].float() + pos[0, 0].float()).to(BF16))
    assert torch.equal(enc.w["pos"], pos[0, 1:])
    # the padded head layout: head h of q / k / v at rows h*128 .. h*128+79, the other 48 zero
    qw, qb = enc.w["0.attn.to_qkv.weight"], enc.w["0.attn.to_qkv.bias"]
    w0, b0 = W[prefix + "visual.transformer.0.attn.to_qkv.weight"], W[prefix + "visual.transformer.0.attn.to_qkv.bias"]
    assert qw.shape == (3 * H * 128, d) and qb.shape == (3 * H * 128,)
    for part in range(3):
        for h in range(H):
            dst, src = (part * H + h) * 128, (part * H + h) * 80
            assert torch.equal(qw[dst:dst + 80], w0[src:src + 80]) and G.bit_zero(qw[dst + 80:dst + 128])
            assert torch.equal(qb[dst:dst + 80], b0[src:src + 80]) and G.bit_zero(qb[dst + 80:dst + 128])
    pw_ = enc.w["0.attn.proj.weight"]
    p0 = W[prefix + "visual.transformer.0.attn.proj.weight"]
    assert pw_.shape == (d, H * 128) and pw_.is_contiguous()
    for h in range(H):
        assert torch.equal(pw_[:, h * 128:h * 128 + 80], p0[:, h * 80:(h + 1) * 80])
        assert G.bit_zero(pw_[:, h * 128 + 80:(h + 1) * 128])


def test_load_state_dict_errors():
    from vstyler.clip import WanImageEncoder
    cfg = C.TINY17
    W = C.random_weights(cfg)
    enc = WanImageEncoder(device="cpu", **cfg)
    missing = {k: v for k, v in W.items() if k != "visual.transformer.1.mlp.2.bias"}
    with pytest.raises(KeyError, match="mlp.2.bias"):
        enc.load_state_dict(missing)
    # the last block is not read: a file without it loads
    enc.load_state_dict({k: v for k, v in W.items() if not k.startswith("visual.transformer.2.")})
    with pytest.raises(KeyError, match="unexpected"):
        enc.load_state_dict(dict(W, **{"visual.transformer.0.attn.q.weight": torch.zeros(2)}))
    with pytest.raises(ValueError, match="pos_embedding"):
        enc.load_state_dict(dict(W, **{"visual.pos_embedding": torch.zeros(1, 257, 320)}))
    assert set(enc.state_dict_shapes()) <= set(W)
    with pytest.raises(NotImplementedError):
        WanImageEncoder(dim=256, num_heads=4, device="cpu")
    with pytest.raises(NotImplementedError):
        WanImageEncoder(dim=80, num_heads=1, device="cpu")            # dim % 64
    with pytest.raises(NotImplementedError):
        WanImageEncoder(patch_size=16, device="cpu")
    with pytest.raises(RuntimeError, match="no weights"):
        WanImageEncoder(device="cpu", **cfg).encode_image(torch.zeros(1, 3, 8, 8, dtype=BF16))


def test_reexport():
    from diffsynth.models.wan_video_image_encoder import WanImageEncoder
    from vstyler import clip
    assert WanImageEncoder is clip.WanImageEncoder


# ------------------------------------------------------------------------------------------- pipeline
class StubEncoder:
    def __init__(self):
        self.calls = []

    def encode_image(self, videos):
        self.calls.append([tuple(v.shape) for v in videos])
        return torch.full((1, 257, 1280), float(len(self.calls)), dtype=BF16)


def _pipe(image=True, pos=False, clip=True):
    """A CPU pipeline whose device-side steps are stubs: the frames, y and the denoise loop (which records
    the clip_feature it is handed)."""
    import i2v_util as I
    from vstyler import WanVideoPipeline
    from vstyler.models import WanModel
    cfg = I.tiny_cfg(num_layers=1, has_image_input=image, has_image_pos_emb=pos)
    pipe = WanVideoPipeline(device="cpu")
    pipe.dit = WanModel(dim=cfg["dim"], in_dim=36, ffn_dim=cfg["ffn_dim"], out_dim=16, text_dim=4096, freq_dim=256,
                        eps=1e-6, patch_size=(1, 2, 2), num_heads=2, num_layers=1, has_image_input=image,
                        has_image_pos_emb=pos, require_clip_embedding=clip, device="meta")
    pipe.image_encoder = StubEncoder()
    seen = {}
    pipe._image_frame = lambda img, name, h, w: torch.zeros(1, 3, 1, h, w, dtype=BF16)
    pipe.encode_input_image = lambda *a, **k: "y"

    def denoise(start, *a, **kw):
        seen.update(kw)
        return start
    pipe.denoise = denoise
    return pipe, seen


def _run(pipe, **kw):
    img = torch.zeros(64, 96, 3, dtype=torch.uint8)
    emb = torch.zeros(1, 64, 4096, dtype=BF16)
    return pipe(prompt_emb=emb, negative_prompt_emb=emb, input_image=img, height=64, width=96, num_frames=5,
                output_type="latents", seed=0, **kw)


def test_pipeline_runs_the_encoder_once_without_end_image():
    pipe, seen = _pipe()
    _run(pipe)
    assert pipe.image_encoder.calls == [[(1, 3, 64, 96)]]
    assert seen["clip_feature"].shape == (1, 257, 1280) and seen["y"] == "y"


def test_pipeline_end_image_joins_only_with_image_pos_emb():
    img2 = torch.zeros(64, 96, 3, dtype=torch.uint8)
    pipe, seen = _pipe(pos=False)
    _run(pipe, end_image=img2)
    assert len(pipe.image_encoder.calls) == 1 and seen["clip_feature"].shape == (1, 257, 1280)
    pipe, seen = _pipe(pos=True)
    _run(pipe, end_image=img2)
    assert len(pipe.image_encoder.calls) == 2 and seen["clip_feature"].shape == (1, 514, 1280)
    assert float(seen["clip_feature"][0, 0, 0]) == 1 and float(seen["clip_feature"][0, 257, 0]) == 2


def test_pipeline_explicit_clip_feature_wins():
    pipe, seen = _pipe()
    mine = torch.full((1, 257, 1280), 7.0, dtype=BF16)
    _run(pipe, clip_feature=mine)
    assert pipe.image_encoder.calls == [] and seen["clip_feature"] is mine


def test_pipeline_skips_the_encoder_without_require_clip_embedding():
    pipe, seen = _pipe(image=False, clip=False)
    _run(pipe)
    assert pipe.image_encoder.calls == [] and seen["clip_feature"] is None


def test_pipeline_without_an_encoder_keeps_its_error():
    pipe, _ = _pipe()
    pipe.image_encoder = None
    with pytest.raises(ValueError, match="clip_feature="):
        _run(pipe)
    with pytest.raises(RuntimeError, match="image_encoder"):
        pipe.encode_clip_image(None, None, 64, 96)


# -------------------------------------------------------------------------------------- preprocessing
@pytest.mark.parametrize("size", C.EXACT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_preprocess_restatement_equals_torch_on_exact_images(size):
    """Source sizes 224 m with pixel values k / 64: t is 0 or 1/2 (weights 1, or -3/32 and 19/32), every
    product and sum is exact in fp32, so torch's fp32 path and the float64 restatement agree to the bit --
    on the interpolated value and after the five roundings."""
    u = C.exact_image(2, *size, seed=3)
    r = C.interp64(u)
    f = F.interpolate(u.float(), size=(224, 224), mode="bicubic", align_corners=False)
    assert torch.equal(r, f.double())
    assert G.same_bits(C.preprocess(u), C.rest(f))
    cols = C.im2col(C.preprocess(u))
    assert cols.shape == (2 * 256, 588)
    xn = C.preprocess(u)
    assert cols[256 + 3 * 16 + 5, 2 * 196 + 4 * 14 + 9] == xn[1, 2, 14 * 3 + 4, 14 * 5 + 9]


@pytest.mark.parametrize("case", range(len(C.INTERVAL_SIZES)), ids=lambda i: "x".join(map(str, C.INTERVAL_SIZES[i])))
def test_preprocess_interval_precondition(case):
    """The interval test's condition, from the reference alone: [rest(r - delta), rest(r + delta)] holds
    more than one bf16 value on at most 0.5 % of the elements; rest is monotone (lo <= mid <= hi)."""
    H, W = C.INTERVAL_SIZES[case]
    u = C.sample_images(1, H, W, 40 + case)[0]
    assert u.shape == (1, 3, H, W) and u.dtype == BF16 and float(u.abs().max()) <= 1
    lo, hi = C.interval(u)
    mid = C.preprocess(u)
    assert bool(((lo <= mid) & (mid <= hi)).all())
    wide = (G.bits(lo) != G.bits(hi)).double().mean().item()
    print(f"{H}x{W}: interval wider than one value on {100 * wide:.3f} % of the elements")
    assert wide <= C.MAX_WIDE, wide


def test_cubic_matrix_rows():
    """Rows sum to one; a 1-pixel axis is that pixel; the taps of 448 -> 224 are (-3, 19, 19, -3) / 32."""
    for n_in in (1, 2, 17, 224, 225, 1280):
        m = C.cubic_matrix(n_in, 224)
        assert torch.allclose(m.sum(dim=1), torch.ones(224, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(C.cubic_matrix(1, 224), torch.ones(224, 1, dtype=torch.float64), atol=1e-12)
    m = C.cubic_matrix(448, 224)
    assert m[5, 9:13].tolist() == [-3 / 32, 19 / 32, 19 / 32, -3 / 32] and float(m[5].abs().sum()) == 44 / 32
    assert m[0, :3].tolist() == [19 / 32 - 3 / 32, 19 / 32, -3 / 32]          # clamped taps add up


# ------------------------------------------------------------------------- attention at head width 80
def test_attn80_exact_preconditions():
    """The width-80 exact problem's preconditions from the reference alone, as test_kernel_refs_cpu.py
    asserts them at width 128: bf16(q c) == q at scale float32(ln 2), integer scores, exact partial sums,
    ambiguous share <= ATTN_MAX_AMBIGUOUS."""
    B, H, S = 2, 3, C.ATTN80_S
    q, k, v = C.attn80_exact_inputs(B, S, H, seed=7)
    assert q.shape == (B * S, H * 80)
    ref, amb, r = C.attn80_exact_ref(q, k, v, H, B)
    share = G.attn_exact_preconditions(r, amb)
    print(f"width 80, s = {S}: ambiguous share {share:.5f}")
    # the padded layout computes the same problem: gpu_util's width-128 reference on it agrees to the bit
    qp, kp, vp = (C.pad_heads(t, H) for t in (q, k, v))
    r128 = G.attn_ref64(qp, kp, vp, H, B, G.ATTN_EXACT_SCALE, exact=True)
    val, pad = C.unpad_heads(r128["o"], H)
    assert torch.equal(val, r["o"]) and bool((pad == 0).all())
    assert torch.equal(r128["l"], r["l"])
