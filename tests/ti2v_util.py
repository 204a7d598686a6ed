"""Test-side restatement of the Wan2.2-TI2V-5B image-to-video mode (fuse_vae_embedding_in_latents with
seperated_timestep), composed from oracle.wan_oracle's pieces as tests/i2v_util.py is.  It follows the
reference's LITERAL per-token path: the timestep vector of length S (wan_video_new.py:1339-1343), t as
[1, S, D] and t_mod as [1, S, 6, D] (:1344, :1349), the block's chunk(dim=2) branch
(wan_video_dit.py:214-229) and the head's 3-D branch (:262-265) -- not the two-row form the product uses.
Arithmetic follows the oracle's convention: fp32 (O.ACC_DTYPE in linear / attention) with a bf16 rounding
wherever the reference materialises a bf16 tensor.  Never used by the product path."""
import torch

from oracle import wan_oracle as O

BF16 = torch.bfloat16

# the tiny TI2V config of the tests: the oracle's "tiny" widths, 48 latent channels in and out
TINY_TI2V = dict(O.WAN_CONFIGS["tiny"], in_dim=48, out_dim=48, num_layers=2, vace_layers=())

# Wan-AI/Wan2.2-TI2V-5B (wan_video_dit.py:678-696)
TI2V_5B = dict(dim=3072, ffn_dim=14336, num_heads=24, num_layers=30, in_dim=48, out_dim=48, text_dim=4096,
               freq_dim=256, eps=1e-6, vace_layers=(), vace_in_dim=96)
TI2V_5B_HASH = "1f5ab7703c6fc803fdded85ff040c316"


def random_weights(cfg=TINY_TI2V, seed=5):
    return O.random_weights(cfg, seed=seed, vace=False)


def inputs(cfg=TINY_TI2V, T=3, h=8, w=12, seed=21):
    """latents (1, 48, T, h, w), first-frame latents (1, 48, 1, h, w), two contexts (1, 64 tokens, 40 / 24 valid)."""
    g = torch.Generator("cpu").manual_seed(seed)
    lat = torch.randn((1, cfg["in_dim"], T, h, w), generator=g).to(BF16)
    first = torch.randn((1, cfg["in_dim"], 1, h, w), generator=g).to(BF16)

    def ctx(n_valid):
        c = 0.1 * torch.randn((1, 64, cfg["text_dim"]), generator=g)
        c[:, n_valid:] = 0
        return c.to(BF16)
    return lat, first, ctx(40), ctx(24)


def token_timesteps(latents, timestep, first=0.0):
    """wan_video_new.py:1340-1343: zeros for the (h/2)(w/2) tokens of latent frame 0, `timestep` for every
    other token, in the latents' dtype.  first: the value of frame 0's tokens (0 in the reference; the
    yardstick's own check forces it to `timestep`)."""
    n0 = latents.shape[3] * latents.shape[4] // 4
    return torch.cat([torch.full((1, n0), float(first), dtype=latents.dtype),
                      torch.ones((latents.shape[2] - 1, n0), dtype=latents.dtype) * timestep.to(latents.dtype)]).flatten()


def dit_block_seq(x, ctx, t_mod, freqs, W, p, num_heads, eps=1e-6):
    """DiTBlock.forward with a 4-D t_mod [1, S, 6, D] (wan_video_dit.py:215-229): chunk(6, dim=2), squeeze(2)."""
    mod = O.bf(W[p + "modulation"].float() + t_mod.float())              # (1,6,D) + (1,S,6,D), :218-219
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = [c.squeeze(2) for c in mod.chunk(6, dim=2)]
    h = O.modulate(O.layer_norm(x, eps), shift_msa, scale_msa)
    x = O.gate_residual(x, gate_msa, O.self_attention(h, freqs, W, p + "self_attn.", num_heads, eps))
    h = O.layer_norm(x, eps, W[p + "norm3.weight"], W[p + "norm3.bias"])
    x = O.add(x, O.cross_attention(h, ctx, W, p + "cross_attn.", num_heads, eps))
    h = O.modulate(O.layer_norm(x, eps), shift_mlp, scale_mlp)
    f = O.blk_linear(O.gelu_tanh(O.blk_linear(h, W[p + "ffn.0.weight"], W[p + "ffn.0.bias"])),
                     W[p + "ffn.2.weight"], W[p + "ffn.2.bias"])
    return O.gate_residual(x, gate_mlp, f)


def head_seq(x, t, W, eps=1e-6):
    """Head.forward, the 3-D branch (wan_video_dit.py:263-265): t [1, S, D]."""
    mod = O.bf(W["head.modulation"].float().unsqueeze(0) + t.float().unsqueeze(2))      # (1,S,2,D)
    shift, scale = [c.squeeze(2) for c in mod.chunk(2, dim=2)]
    return O.linear(O.modulate(O.layer_norm(x, eps), shift, scale), W["head.head.weight"], W["head.head.bias"])


def model_fn(W, cfg, latents, timestep, context, first=0.0):
    """model_fn_wan_video with dit.seperated_timestep and fuse_vae_embedding_in_latents (wan_video_new.py
    :1339-1349, then :1357-1468 without VACE): latents of batch 1 repeated to the context's batch."""
    D, H, eps = cfg["dim"], cfg["num_heads"], cfg["eps"]
    B = context.shape[0]
    ts = token_timesteps(latents, timestep.reshape(()), first)                         # (S,)
    t, t_mod = O.time_embed(ts, W, D)                                                   # rows = tokens
    t, t_mod = t.unsqueeze(0), t_mod.unsqueeze(0)                                       # (1,S,D), (1,S,6,D)
    ctx = O.text_embed(context, W)
    x = latents.expand(B, *latents.shape[1:]) if latents.shape[0] != B else latents
    x, (f, h, w) = O.patchify(x, W["patch_embedding.weight"], W["patch_embedding.bias"])
    freqs = O.rope_freqs(f, h, w, D // H)
    for i in range(cfg["num_layers"]):
        x = dit_block_seq(x, ctx, t_mod, freqs, W, f"blocks.{i}.", H, eps)
    x = head_seq(x, t, W, eps)
    return O.unpatchify(x, (f, h, w), cfg["out_dim"])


def denoise(W, cfg, latents, first_frame, context_pos, context_neg, num_inference_steps=2, cfg_scale=5.0,
            sigma_shift=5.0):
    """The Euler loop of wan_video_new.py:515-542 with the first-frame pin: frame 0 of the start latents is
    the clean first frame (:747) and is set back to it after every scheduler step (:541-542)."""
    sigmas, timesteps = O.set_timesteps(num_inference_steps, 1.0, sigma_shift)
    latents = latents.clone()
    latents[:, :, 0:1] = first_frame
    for i, ts in enumerate(timesteps):
        t = ts.unsqueeze(0).to(BF16)
        vp = model_fn(W, cfg, latents, t, context_pos)
        vn = model_fn(W, cfg, latents, t, context_neg)
        latents = O.cfg_euler(vp, vn, latents, cfg_scale, O.euler_delta(sigmas, i))
        latents[:, :, 0:1] = first_frame
    return latents


def with_float64(fn):
    """fn() with the oracle's linear / attention accumulating in float64: the floor restatement."""
    old = O.ACC_DTYPE
    O.ACC_DTYPE = torch.float64
    try:
        return fn()
    finally:
        O.ACC_DTYPE = old


def build(cfg, W, device="cuda", fused=True):
    """The product WanModel of cfg with W loaded (strict)."""
    from vstyler.models import WanModel
    dit = WanModel(dim=cfg["dim"], in_dim=cfg["in_dim"], ffn_dim=cfg["ffn_dim"], out_dim=cfg["out_dim"], text_dim=4096,
                   freq_dim=256, eps=1e-6, patch_size=(1, 2, 2), num_heads=cfg["num_heads"],
                   num_layers=cfg["num_layers"], seperated_timestep=fused, fuse_vae_embedding_in_latents=fused,
                   require_clip_embedding=False, require_vae_embedding=False, device=device)
    if W is not None:
        dit.load_state_dict(W, strict=True)
    return dit
