"""Test-side restatement of the image-conditioned (I2V / FLF2V / Fun-InP) parts of the Wan DiT, composed
from oracle.wan_oracle's pieces (the oracle itself covers the T2V / VACE layout only).  Every function
cites the reference lines it restates (diffsynth/models/wan_video_dit.py, diffsynth/pipelines/
wan_video_new.py).  Arithmetic follows the oracle's convention: fp32 (O.ACC_DTYPE in linear / attention)
with a bf16 rounding wherever the reference materialises a bf16 tensor.  Never used by the product path."""
import torch
import torch.nn.functional as F

from oracle import wan_oracle as O

BF16 = torch.bfloat16
CLIP_DIM = 1280
IMG_TOKENS = 257

# the tiny image-conditioned configs of the GPU tests: the oracle's "tiny" widths, in_dim 36
TINY_I2V = dict(O.WAN_CONFIGS["tiny"], in_dim=36, num_layers=2, vace_layers=())


def tiny_cfg(num_layers=2, has_image_input=True, has_image_pos_emb=False):
    return dict(TINY_I2V, num_layers=num_layers, has_image_input=has_image_input,
                has_image_pos_emb=has_image_pos_emb)


def image_param_shapes(cfg):
    """The parameters WanModel(has_image_input=True) adds: MLP(1280, dim, has_pos_emb) as img_emb
    (wan_video_dit.py:232-244, :321-322) and k_img / v_img / norm_k_img of every block's CrossAttention
    (:164-167)."""
    D = cfg["dim"]
    s = {"img_emb.proj.0.weight": (CLIP_DIM,), "img_emb.proj.0.bias": (CLIP_DIM,),
         "img_emb.proj.1.weight": (CLIP_DIM, CLIP_DIM), "img_emb.proj.1.bias": (CLIP_DIM,),
         "img_emb.proj.3.weight": (D, CLIP_DIM), "img_emb.proj.3.bias": (D,),
         "img_emb.proj.4.weight": (D,), "img_emb.proj.4.bias": (D,)}
    if cfg.get("has_image_pos_emb"):
        s["img_emb.emb_pos"] = (1, 2 * IMG_TOKENS, CLIP_DIM)
    for i in range(cfg["num_layers"]):
        p = f"blocks.{i}.cross_attn."
        s[p + "k_img.weight"] = (D, D)
        s[p + "k_img.bias"] = (D,)
        s[p + "v_img.weight"] = (D, D)
        s[p + "v_img.bias"] = (D,)
        s[p + "norm_k_img.weight"] = (D,)
    return s


def random_weights(cfg, seed=5):
    """O.random_weights (no VACE) for cfg's in_dim, plus, for has_image_input, the image parameters from a
    generator of their own (seed + 1000), by the oracle's init rule; the two LayerNorm weights of
    img_emb.proj (names without "norm") get the norm rule too, emb_pos N(0, 0.02)."""
    W = O.random_weights(cfg, seed=seed, vace=False)
    if cfg.get("has_image_input"):
        gen = torch.Generator("cpu").manual_seed(seed + 1000)
        for k, shape in image_param_shapes(cfg).items():
            name = "norm." + k if k in ("img_emb.proj.0.weight", "img_emb.proj.4.weight") else k
            W[k] = O.init_weight(name, shape, gen, cfg["dim"])
    return W


def inputs(cfg, T=3, h=8, w=12, batch=1, clip_rows=IMG_TOKENS, seed=11):
    """latents (batch, 16, T, h, w), y (1, in_dim - 16, T, h, w) = [4 mask channels in {0, 1} | N(0, 1)],
    clip_feature (1, clip_rows, 1280) ~ N(0, 1), two contexts (batch 1, 64 tokens, 40 / 24 valid)."""
    g = torch.Generator("cpu").manual_seed(seed)
    lat = torch.randn((batch, 16, T, h, w), generator=g).to(BF16)
    cy = cfg["in_dim"] - 16
    y = torch.randn((1, cy, T, h, w), generator=g)
    y[:, :4] = (torch.rand((1, 4, T, 1, 1), generator=g) < 0.5).float().expand(1, 4, T, h, w)
    clip = torch.randn((1, clip_rows, CLIP_DIM), generator=g).to(BF16)

    def ctx(n_valid):
        c = 0.1 * torch.randn((1, 64, cfg["text_dim"]), generator=g)
        c[:, n_valid:] = 0
        return c.to(BF16)
    return lat, y.to(BF16), clip, ctx(40), ctx(24)


def gelu_erf(x):
    """nn.GELU() (wan_video_dit.py:239) on a bf16 tensor: the erf form, one rounding."""
    return O.bf(F.gelu(x.float()))


def img_emb(clip_feature, W, cfg, eps=1e-5):
    """MLP.forward (wan_video_dit.py:246-249): [x + emb_pos,] LayerNorm(1280), Linear, GELU, Linear,
    LayerNorm(dim) -- nn.LayerNorm's default eps 1e-5, each module's output a bf16 tensor."""
    x = clip_feature
    if cfg.get("has_image_pos_emb"):
        x = O.add(x, W["img_emb.emb_pos"])                                          # :247-248
    x = O.layer_norm(x, eps, W["img_emb.proj.0.weight"], W["img_emb.proj.0.bias"])
    x = gelu_erf(O.linear(x, W["img_emb.proj.1.weight"], W["img_emb.proj.1.bias"]))
    x = O.linear(x, W["img_emb.proj.3.weight"], W["img_emb.proj.3.bias"])
    return O.layer_norm(x, eps, W["img_emb.proj.4.weight"], W["img_emb.proj.4.bias"])


def cross_attention_image(x, y, W, p, num_heads, eps=1e-6):
    """CrossAttention.forward with has_image_input (wan_video_dit.py:171-186): y = cat([image rows,
    text]); img = y[:, :257], ctx = y[:, 257:] (:172-174); x = attn(q, k, v) + attn(q, k_img, v_img) as a
    bf16 add (:181-185); then o."""
    img, ctx = y[:, :IMG_TOKENS], y[:, IMG_TOKENS:]
    q = O.rms_norm(O.blk_linear(x, W[p + "q.weight"], W[p + "q.bias"]), W[p + "norm_q.weight"], eps)
    k = O.rms_norm(O.blk_linear(ctx, W[p + "k.weight"], W[p + "k.bias"]), W[p + "norm_k.weight"], eps)
    v = O.blk_linear(ctx, W[p + "v.weight"], W[p + "v.bias"])
    o = O.attention(q, k, v, num_heads)
    k_img = O.rms_norm(O.linear(img, W[p + "k_img.weight"], W[p + "k_img.bias"]), W[p + "norm_k_img.weight"], eps)
    v_img = O.linear(img, W[p + "v_img.weight"], W[p + "v_img.bias"])
    o = O.add(o, O.attention(q, k_img, v_img, num_heads))
    return O.blk_linear(o, W[p + "o.weight"], W[p + "o.bias"])


def dit_block(x, y, t_mod, freqs, W, p, num_heads, has_image_input, eps=1e-6):
    """DiTBlock.forward (wan_video_dit.py:214-230) with the cross-attention above when has_image_input."""
    if not has_image_input:
        return O.dit_block(x, y, t_mod, freqs, W, p, num_heads, eps)
    mod = O.bf(W[p + "modulation"].float() + t_mod.float())
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = mod.chunk(6, dim=1)
    h = O.modulate(O.layer_norm(x, eps), shift_msa, scale_msa)
    x = O.gate_residual(x, gate_msa, O.self_attention(h, freqs, W, p + "self_attn.", num_heads, eps))
    h = O.layer_norm(x, eps, W[p + "norm3.weight"], W[p + "norm3.bias"])
    x = O.add(x, cross_attention_image(h, y, W, p + "cross_attn.", num_heads, eps))
    h = O.modulate(O.layer_norm(x, eps), shift_mlp, scale_mlp)
    f = O.blk_linear(O.gelu_tanh(O.blk_linear(h, W[p + "ffn.0.weight"], W[p + "ffn.0.bias"])),
                     W[p + "ffn.2.weight"], W[p + "ffn.2.bias"])
    return O.gate_residual(x, gate_mlp, f)


def model_fn(W, cfg, latents, timestep, context, y=None, clip_feature=None):
    """model_fn_wan_video with y / clip_feature (wan_video_new.py:1351-1468, no VACE): x = cat([x, y], 1)
    (:1367-1368), context = cat([img_emb(clip_feature), text], 1) (:1369-1371), patchify, blocks, head.
    latents / y / clip_feature of batch 1 are repeated to the context's batch (:1361-1364)."""
    D, H, eps = cfg["dim"], cfg["num_heads"], cfg["eps"]
    B = context.shape[0]
    t, t_mod = O.time_embed(timestep.expand(B) if timestep.shape[0] != B else timestep, W, D)
    ctx = O.text_embed(context, W)
    x = latents.expand(B, *latents.shape[1:]) if latents.shape[0] != B else latents
    if y is not None:
        x = torch.cat([x, y.expand(B, *y.shape[1:])], dim=1)
    image = bool(cfg.get("has_image_input")) and clip_feature is not None
    if image:
        emb = img_emb(clip_feature, W, cfg)
        ctx = torch.cat([emb.expand(B, *emb.shape[1:]), ctx], dim=1)
    x, (f, h, w) = O.patchify(x, W["patch_embedding.weight"], W["patch_embedding.bias"])
    freqs = O.rope_freqs(f, h, w, D // H)
    for i in range(cfg["num_layers"]):
        x = dit_block(x, ctx, t_mod, freqs, W, f"blocks.{i}.", H, image, eps)
    x = O.head(x, t, W, eps)
    return O.unpatchify(x, (f, h, w), cfg["out_dim"])


def with_float64(fn):
    """fn() with the oracle's linear / attention accumulating in float64: the floor restatement."""
    old = O.ACC_DTYPE
    O.ACC_DTYPE = torch.float64
    try:
        return fn()
    finally:
        O.ACC_DTYPE = old


def build(cfg, W, device="cuda"):
    """The product WanModel of cfg with W loaded (strict)."""
    from vstyler.models import WanModel
    dit = WanModel(dim=cfg["dim"], in_dim=cfg["in_dim"], ffn_dim=cfg["ffn_dim"], out_dim=16, text_dim=4096,
                   freq_dim=256, eps=1e-6, patch_size=(1, 2, 2), num_heads=cfg["num_heads"],
                   num_layers=cfg["num_layers"], has_image_input=bool(cfg.get("has_image_input")),
                   has_image_pos_emb=bool(cfg.get("has_image_pos_emb")), device=device)
    dit.load_state_dict(W, strict=True)
    return dit


# ---------------------------------------------------------------------------- the image embedder unit
def reference_mask_and_vae_input(image, end_image, num_frames, height, width):
    """WanVideoUnit_ImageEmbedderVAE.process, wan_video_new.py:709-720, literally: image / end_image are
    the preprocessed (1, 3, H, W) tensors.  Returns (msk (4, T', h, w), vae_input (3, num_frames, H, W))."""
    msk = torch.ones(1, num_frames, height // 8, width // 8)
    msk[:, 1:] = 0
    if end_image is not None:
        vae_input = torch.concat([image.transpose(0, 1), torch.zeros(3, num_frames - 2, height, width).to(image.dtype),
                                  end_image.transpose(0, 1)], dim=1)
        msk[:, -1:] = 1
    else:
        vae_input = torch.concat([image.transpose(0, 1), torch.zeros(3, num_frames - 1, height, width).to(image.dtype)],
                                 dim=1)
    msk = torch.concat([torch.repeat_interleave(msk[:, 0:1], repeats=4, dim=1), msk[:, 1:]], dim=1)
    msk = msk.view(1, msk.shape[1] // 4, 4, height // 8, width // 8)
    msk = msk.transpose(1, 2)[0]
    return msk, vae_input


# ------------------------------------------------------------------------------- test-side tiler with y
def tile_y(forward, latents, y, size, stride):
    """window_util.tile with y cut by the same [t, t_) (the reference's tiler slices y: its
    tensor_names, wan_video_new.py:1291-1300)."""
    from window_util import tile
    state = {}

    def fwd(lat, _):
        t = state["t"].pop(0)
        return forward(lat, None if y is None else y[:, :, t: t + lat.shape[2]])
    T = latents.shape[2]
    state["t"] = [t for t in range(0, T, stride) if not (t - stride >= 0 and t - stride + size >= T)]
    return tile(fwd, latents, None, size, stride)
