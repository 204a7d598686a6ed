"""Test-side restatement of the Wan-Fun control parts of the Wan DiT and pipeline (reference image through
ref_conv, camera control adapter, the y / clip_feature assembly of the three Fun units, the Pluecker rays),
composed from oracle.wan_oracle's pieces and tests/i2v_util.py as that file is.  Every function cites the
reference lines it restates (diffsynth/models/wan_video_dit.py, diffsynth/models/
wan_video_camera_controller.py, diffsynth/pipelines/wan_video_new.py).  Arithmetic follows the oracle's
convention: O.ACC_DTYPE accumulation with a bf16 rounding wherever the reference's bf16 modules materialise
a tensor.  Never used by the product path."""
import numpy as np
import torch
import torch.nn.functional as F

import i2v_util as I
from oracle import wan_oracle as O

BF16 = torch.bfloat16


def tiny_cfg(in_dim, has_image_input, has_ref_conv=False, add_control_adapter=False, num_layers=2):
    """The tiny DiT of tests/test_i2v_gpu.py (dim 256, 2 heads) with the Fun-Control flags."""
    return dict(I.tiny_cfg(num_layers=num_layers, has_image_input=has_image_input), in_dim=in_dim,
                has_ref_conv=has_ref_conv, add_control_adapter=add_control_adapter, in_dim_control_adapter=24)


def control_param_shapes(cfg):
    """ref_conv = Conv2d(16, dim, 2, 2) (wan_video_dit.py:331); control_adapter = SimpleAdapter(24, dim, 2, 2):
    conv = Conv2d(64 in, dim, 2, 2), residual_blocks.0.conv{1,2} = Conv2d(dim, dim, 3, padding=1)
    (wan_video_camera_controller.py:17-22, 66-68)."""
    D, s = cfg["dim"], {}
    if cfg.get("has_ref_conv"):
        s["ref_conv.weight"], s["ref_conv.bias"] = (D, 16, 2, 2), (D,)
    if cfg.get("add_control_adapter"):
        cin = 64 * cfg.get("in_dim_control_adapter", 24)
        s["control_adapter.conv.weight"], s["control_adapter.conv.bias"] = (D, cin, 2, 2), (D,)
        for n in ("conv1", "conv2"):
            s[f"control_adapter.residual_blocks.0.{n}.weight"] = (D, D, 3, 3)
            s[f"control_adapter.residual_blocks.0.{n}.bias"] = (D,)
    return s


def random_weights(cfg, seed=5):
    """I.random_weights plus the control parameters from a generator of their own (seed + 2000), by the
    oracle's init rule -- with every block's self-attention weights (q, k, v, o) times 4 (exact in bf16).
    Under the plain N(0, 0.02) init the attention branch is so weak beside the residual stream that a
    forward with the reference frame at a wrong RoPE index, or without the reference rows at all, stays
    within the floor's bound (rel-L2 0.0038 / 0.0058 against a bound of 0.0054): a test on that model could
    not tell a wrong token grid from a right one.  Times 4 the wrong grid is 3 x outside the bound
    (tests/test_funcontrol_cpu.py::test_restatement_catches_a_wrong_grid)."""
    W = I.random_weights(cfg, seed=seed)
    for k in W:
        if ".self_attn." in k and k.endswith((".q.weight", ".k.weight", ".v.weight", ".o.weight")):
            W[k] = (W[k].float() * 4).to(BF16)
    gen = torch.Generator("cpu").manual_seed(seed + 2000)
    for k, shape in control_param_shapes(cfg).items():
        W[k] = O.init_weight(k, shape, gen, cfg["dim"])
    return W


def build(cfg, W, device="cuda"):
    from vstyler.models import WanModel
    dit = WanModel(dim=cfg["dim"], in_dim=cfg["in_dim"], ffn_dim=cfg["ffn_dim"], out_dim=16, text_dim=4096,
                   freq_dim=256, eps=1e-6, patch_size=(1, 2, 2), num_heads=cfg["num_heads"],
                   num_layers=cfg["num_layers"], has_image_input=bool(cfg.get("has_image_input")),
                   require_clip_embedding=bool(cfg.get("has_image_input")),
                   has_ref_conv=bool(cfg.get("has_ref_conv")), add_control_adapter=bool(cfg.get("add_control_adapter")),
                   in_dim_control_adapter=cfg.get("in_dim_control_adapter", 24), device=device)
    dit.load_state_dict(W, strict=True)
    return dit


def conv2d(x, w, b, **kw):
    """A bf16 nn.Conv2d: accumulate in O.ACC_DTYPE, + bias, one rounding."""
    return O.bf(F.conv2d(x.to(O.ACC_DTYPE), w.to(O.ACC_DTYPE), b.to(O.ACC_DTYPE), **kw))


def ref_tokens(reference_latents, W):
    """wan_video_new.py:1386-1388: [:, :, 0] of a 5-D tensor, ref_conv, flatten(2).transpose(1, 2)."""
    r = reference_latents
    if len(r.shape) == 5:
        r = r[:, :, 0]
    return conv2d(r, W["ref_conv.weight"], W["ref_conv.bias"], stride=2).flatten(2).transpose(1, 2)


def adapter(cc, W):
    """SimpleAdapter.forward (wan_video_camera_controller.py:24-44) on [bs, c, f, h, w] -> [bs, dim, f, h/16,
    w/16]; ResidualBlock (:70-75): relu(conv1(x)), conv2, out += residual -- every module output bf16."""
    bs, c, f, h, w = cc.shape
    x = cc.permute(0, 2, 1, 3, 4).contiguous().view(bs * f, c, h, w)
    x = F.pixel_unshuffle(x, 8)
    p = "control_adapter."
    x = conv2d(x, W[p + "conv.weight"], W[p + "conv.bias"], stride=2)
    r = p + "residual_blocks.0."
    out = O.bf(F.relu(conv2d(x, W[r + "conv1.weight"], W[r + "conv1.bias"], padding=1).float()))
    out = conv2d(out, W[r + "conv2.weight"], W[r + "conv2.bias"], padding=1)
    out = O.add(out, x)
    out = out.view(bs, f, out.size(1), out.size(2), out.size(3))
    return out.permute(0, 2, 1, 3, 4)


def model_fn(W, cfg, latents, timestep, context, y=None, clip_feature=None, reference_latents=None,
             control_camera_latents_input=None, ref_rope_index=None):
    """model_fn_wan_video (wan_video_new.py:1351-1468, no VACE) with the reference image (:1385-1390: concat
    in front, f += 1; :1464-1465: drop the rows after the head) and camera control (wan_video_dit.py:339-345:
    patch embedding + adapter, a bf16 add).  Without either it is i2v_util.model_fn line for line.
    ref_rope_index: a WRONG variant for the yardstick's own check -- the reference frame's temporal RoPE
    index moved from 0 to that value (and the video frames' to 0..f-1)."""
    D, H, eps = cfg["dim"], cfg["num_heads"], cfg["eps"]
    B = context.shape[0]
    t, t_mod = O.time_embed(timestep.expand(B) if timestep.shape[0] != B else timestep, W, D)
    ctx = O.text_embed(context, W)
    x = latents.expand(B, *latents.shape[1:]) if latents.shape[0] != B else latents
    if y is not None:
        x = torch.cat([x, y.expand(B, *y.shape[1:])], dim=1)
    image = bool(cfg.get("has_image_input")) and clip_feature is not None
    if image:
        emb = I.img_emb(clip_feature, W, cfg)
        ctx = torch.cat([emb.expand(B, *emb.shape[1:]), ctx], dim=1)
    x, (f, h, w) = O.patchify(x, W["patch_embedding.weight"], W["patch_embedding.bias"])
    if control_camera_latents_input is not None:
        cam = adapter(control_camera_latents_input, W)                        # [1, D, f, h, w]
        cam = cam.permute(0, 2, 3, 4, 1).reshape(1, f * h * w, D)             # the rearrange of :1382
        x = O.add(x, cam.expand(B, f * h * w, D))
    n = 0
    if reference_latents is not None:
        r = ref_tokens(reference_latents, W)
        n = r.shape[1]
        x = torch.cat([r.expand(B, n, D), x], dim=1)
        f += 1
    freqs = O.rope_freqs(f, h, w, D // H)
    if ref_rope_index is not None:
        fr = O.rope_freqs(max(f, ref_rope_index + 1), h, w, D // H)
        freqs = torch.cat([fr[ref_rope_index * h * w:(ref_rope_index + 1) * h * w], fr[:(f - 1) * h * w]])
    for i in range(cfg["num_layers"]):
        x = I.dit_block(x, ctx, t_mod, freqs, W, f"blocks.{i}.", H, image, eps)
    x = O.head(x, t, W, eps)
    if reference_latents is not None:
        x = x[:, n:]
        f -= 1
    return O.unpatchify(x, (f, h, w), cfg["out_dim"])


# ------------------------------------------------------------------------- the three units' y assembly
def fun_control(control_latents, clip_feature, y, in_dim, num_frames, height, width):
    """WanVideoUnit_FunControl.process, wan_video_new.py:766-773, literally (latents have 16 channels)."""
    y_dim = in_dim - control_latents.shape[1] - 16
    if clip_feature is None or y is None:
        clip_feature = torch.zeros((1, 257, 1280), dtype=BF16)
        y = torch.zeros((1, y_dim, (num_frames - 1) // 4 + 1, height // 8, width // 8), dtype=BF16)
    else:
        y = y[:, -y_dim:]
    y = torch.concat([control_latents, y], dim=1)
    return {"clip_feature": clip_feature, "y": y}


def camera_y(input_latents, mask_form, in_dim, num_frames, height, width):
    """WanVideoUnit_FunCameraControl.process, wan_video_new.py:828-844: y = zeros_like(latents) with the
    encoded image in frame 0; when that is not in_dim - 16 channels, the mask + latents form (mask_form():
    the encode of [image, zeros] under the four mask channels, i2v_util.reference_mask_and_vae_input)."""
    y = torch.zeros((1, 16, (num_frames - 1) // 4 + 1, height // 8, width // 8), dtype=BF16)
    y[:, :, :1] = input_latents
    if y.shape[1] != in_dim - 16:
        y = mask_form()
    return y


def group_in_fours(plucker, num_frames):
    """wan_video_new.py:813-822: plucker [F, H, W, 6] -> control_camera_latents_input [1, 24, T, H, W]."""
    v = plucker[:num_frames].permute([3, 0, 1, 2]).unsqueeze(0)
    lat = torch.concat([torch.repeat_interleave(v[:, :, 0:1], repeats=4, dim=2), v[:, :, 1:]], dim=2).transpose(1, 2)
    b, f, c, h, w = lat.shape
    lat = lat.contiguous().view(b, f // 4, 4, c, h, w).transpose(2, 3)
    return lat.contiguous().view(b, f // 4, c * 4, h, w).transpose(1, 2)


# ---------------------------------------------------------------------------------- Pluecker rays, float64
def plucker64(intrinsics, c2w, height, width):
    """ray_condition (wan_video_camera_controller.py:114-147) in float64 on the fp32 matrices the host
    hands the kernel: intrinsics [F, 4] = (fx, fy, cx, cy) in pixels, c2w [F, 3, 4] -> [F, H, W, 6]
    (moment o x d, direction d)."""
    k = np.asarray(intrinsics, dtype=np.float64)
    m = np.asarray(c2w, dtype=np.float64)
    jj, ii = np.meshgrid(np.arange(height, dtype=np.float64) + 0.5, np.arange(width, dtype=np.float64) + 0.5,
                         indexing="ij")
    out = np.empty((k.shape[0], height, width, 6))
    for f in range(k.shape[0]):
        fx, fy, cx, cy = k[f]
        d = np.stack([(ii - cx) / fx, (jj - cy) / fy, np.ones_like(ii)], axis=-1)
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        rays_d = d @ m[f, :, :3].T
        rays_o = np.broadcast_to(m[f, :, 3], rays_d.shape)
        out[f, ..., :3] = np.cross(rays_o, rays_d)
        out[f, ..., 3:] = rays_d
    return out


def fixture():
    """tests/golden/camera_plucker.npz as {case: (direction, speed, origin or None, fp32 [5, 16, 32, 6])}."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_plucker.npz"))
    out = {}
    for name in ("left", "rightdown", "leftup_rot"):
        origin = tuple(float(v) for v in d[name + "_origin"]) or None
        out[name] = (str(d[name + "_direction"]), float(d[name + "_speed"]), origin, d[name])
    return out


# the fp32 slack of the camera-ray checks: 4 x the largest |reference fp32 - float64 restatement| over the
# fixture cases and one 480x832 frame.  Measured on the CPU: 1.27, 1.27, 1.87 (the three fixture cases) and
# 1.91 ("Left"), 2.68 ("LeftUp" with the fixture's rotated origin) at 480x832, in units of 2^-24; 2.7 * 2^-24
# it is.  tests/test_funcontrol_cpu.py holds the fixture cases to it; the margin of 4 covers another fp32
# operation order (fma, a reciprocal square root).
MEASURED_FP32_DIFF = 2.7 * 2.0 ** -24
RAY_SLACK = 4 * MEASURED_FP32_DIFF
