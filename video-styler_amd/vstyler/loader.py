"""Checkpoint loading with the reference's model detection (md5 of sorted 'key:shape' strings).

Reference: diffsynth/models/utils.py:65-88 (readers), :148-182 (hash), diffsynth/models/
model_manager.py:162-196 (detector), configs/model_config.py:142-179 (hash table),
wan_video_dit.py:506-536 / wan_video_vace.py:98-113 (hash -> config).  Serialized files are read
with safetensors or torch.load(weights_only=True) only.
"""
import hashlib
import os

import torch

from .models import ANIMATE_PREFIXES, DiTBlock, VaceWanModel, WanAnimateAdapter, WanModel, block_fp8_linears

WAN_DIT_CONFIGS = {
    "9269f8db9040a9d860eaca435be61814": dict(dim=1536, ffn_dim=8960, num_heads=12, num_layers=30),   # 1.3B
    "aafcfd9672c3a2456dc46e1cb6e52c70": dict(dim=5120, ffn_dim=13824, num_heads=40, num_layers=40),  # 14B
}
# The image-conditioned layouts (wan_video_dit.py:537-712): in_dim = 16 + the y channels.  A table of its
# own, looked up after the one above (whose size tests/test_oracle_kat.py pins).
WAN_I2V_DIT_CONFIGS = {
    "6bfcfb3b342cb286ce886889d519a77e": dict(dim=5120, ffn_dim=13824, num_heads=40, num_layers=40, in_dim=36,
                                             has_image_input=True),                          # I2V-14B
    "6d6ccde6845b95ad9114ab993d917893": dict(dim=1536, ffn_dim=8960, num_heads=12, num_layers=30, in_dim=36,
                                             has_image_input=True),                          # Fun-1.3B-InP
    "3ef3b1f8e1dab83d5b71fd7b617f859f": dict(dim=5120, ffn_dim=13824, num_heads=40, num_layers=40, in_dim=36,
                                             has_image_input=True, has_image_pos_emb=True),  # FLF2V-14B
    "5b013604280dd715f8457c6ed6d6a626": dict(dim=5120, ffn_dim=13824, num_heads=40, num_layers=40, in_dim=36,
                                             has_image_input=False, require_clip_embedding=False),  # Wan2.2-I2V-A14B
    "349723183fc063b2bfc10bb2835cf677": dict(dim=1536, ffn_dim=8960, num_heads=12, num_layers=30, in_dim=48,
                                             has_image_input=True),                          # Fun-1.3B-Control
}
# Wan2.2-TI2V-5B (wan_video_dit.py:678-696): 48 latent channels in and out, no y and no CLIP branch; in
# its image-to-video mode the clean first-frame latents sit in latent frame 0, whose tokens run at
# timestep 0 (seperated_timestep / fuse_vae_embedding_in_latents).  A third table, looked up last.
WAN_TI2V_DIT_CONFIGS = {
    "1f5ab7703c6fc803fdded85ff040c316": dict(dim=3072, ffn_dim=14336, num_heads=24, num_layers=30, in_dim=48,
                                             out_dim=48, has_image_input=False, seperated_timestep=True,
                                             require_clip_embedding=False, require_vae_embedding=False,
                                             fuse_vae_embedding_in_latents=True),
}
# Wan-Fun control (wan_video_dit.py:580-594, 610-677, 713-748): control latents in y (in_dim 48 / 52), the
# reference image's ref_conv, the camera control_adapter (in_dim 32 / 36).  A fourth table, looked up after
# the three above.
_B13 = dict(dim=1536, ffn_dim=8960, num_heads=12, num_layers=30)
_B14 = dict(dim=5120, ffn_dim=13824, num_heads=40, num_layers=40)
WAN_FUN_DIT_CONFIGS = {
    "efa44cddf936c70abd0ea28b6cbe946c": dict(_B14, in_dim=48, has_image_input=True),         # 14B control v1.0
    "70ddad9d3a133785da5ea371aae09504": dict(_B13, in_dim=48, has_image_input=True, has_ref_conv=True),   # 1.3B v1.1
    "26bde73488a92e64cc20b0a7485b9e5b": dict(_B14, in_dim=48, has_image_input=True, has_ref_conv=True),   # 14B v1.1
    "ac6a5aa74f4a0aab6f64eb9a72f19901": dict(_B13, in_dim=32, has_image_input=True, add_control_adapter=True,
                                             in_dim_control_adapter=24),                     # 1.3B camera v1.1
    "b61c605c2adbd23124d152ed28e049ae": dict(_B14, in_dim=32, has_image_input=True, add_control_adapter=True,
                                             in_dim_control_adapter=24),                     # 14B camera v1.1
    "2267d489f0ceb9f21836532952852ee5": dict(_B14, in_dim=52, has_image_input=False, has_ref_conv=True,
                                             require_clip_embedding=False),                  # Wan2.2-Fun-A14B-Control
    "47dbeab5e560db3180adf51dc0232fb1": dict(_B14, in_dim=36, has_image_input=False, add_control_adapter=True,
                                             in_dim_control_adapter=24,
                                             require_clip_embedding=False),           # Wan2.2-Fun-A14B-Control-Camera
}
# Wan2.2-Animate-14B (configs/model_config.py:179): the I2V-14B DiT's key set plus the adapter's 138 keys.  The
# file is split as the reference's two converters split it (wan_video_dit.py:508,
# wan_video_animate_adapter.py:664-669): the DiT part is looked up in the tables above.
WAN_ANIMATE_HASH = "31fa352acb8a1b1d33cd8764273d80a2"
WAN_COMMON = dict(in_dim=16, out_dim=16, text_dim=4096, freq_dim=256, eps=1e-6, patch_size=(1, 2, 2))
VACE_14B_HASH = "3b2726384e4f64837bdf216eea3f310d"
VACE_14B = dict(vace_layers=(0, 5, 10, 15, 20, 25, 30, 35), vace_in_dim=96, patch_size=(1, 2, 2),
                dim=5120, num_heads=40, ffn_dim=13824, eps=1e-6)
MAIN_LAYERS_BY_DIM = {1536: 30, 5120: 40}
VACE_DEFAULT = dict(vace_layers=tuple(range(0, 30, 2)), vace_in_dim=96, patch_size=(1, 2, 2),
                    dim=1536, num_heads=12, ffn_dim=8960, eps=1e-6)   # VaceWanModel() defaults


def hash_state_dict_keys(state_dict, with_shape=True):
    """models/utils.py:148-182."""
    keys = []
    for key, value in state_dict.items():
        if isinstance(key, str) and isinstance(value, torch.Tensor):
            if with_shape:
                keys.append(key + ":" + "_".join(map(str, list(value.shape))))
            keys.append(key)
    keys.sort()
    return hashlib.md5(",".join(keys).encode("UTF-8")).hexdigest()


def load_state_dict(path, device="cpu", torch_dtype=None):
    if isinstance(path, (list, tuple)):
        sd = {}
        for p in path:
            sd.update(load_state_dict(p, device, torch_dtype))
        return sd
    if os.path.isdir(path):
        sd = {}
        for name in sorted(os.listdir(path)):
            if name.split(".")[-1] in ("safetensors", "bin", "ckpt", "pth", "pt"):
                sd.update(load_state_dict(os.path.join(path, name), device, torch_dtype))
        return sd
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(path, device=str(device))
    else:
        sd = torch.load(path, map_location=device, weights_only=True)
    if torch_dtype is not None:
        sd = {k: (v.to(torch_dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
              for k, v in sd.items()}
    return sd


_PREFIXES = ("model.diffusion_model.", "diffusion_model.")


def normalize_keys(state_dict):
    """ComfyUI / Kijai WanVideo checkpoints (the config-5 workflow's model files) carry the Wan key
    layout under a 'model.diffusion_model.' or 'diffusion_model.' prefix, fp8 e4m3fn linear weights
    and, in their '_scaled' variants, per-tensor '<name>.scale_weight' factors.  Strip the prefix and
    fold scale_weight into its weight (exact fp8 -> bf16 upcast, then the scale) so the reference's
    md5 key-layout detection applies unchanged.  Other layouts pass through."""
    sd = {}
    for k, v in state_dict.items():
        for pre in _PREFIXES:
            if k.startswith(pre):
                k = k[len(pre):]
                break
        sd[k] = v
    for k in [k for k in sd if k.endswith(".scale_weight")]:
        base = k[: -len(".scale_weight")] + ".weight"
        s = sd.pop(k)
        if base in sd:
            sd[base] = (sd[base].to(torch.float32) * s.to(torch.float32)).to(torch.bfloat16)
    sd.pop("scaled_fp8", None)
    return sd


def fp8_checkpoint_tensors(state_dict):
    """The float8_e4m3fn '<name>.weight' tensors of a checkpoint as it is on disk: {'<name>' (prefix
    stripped): (e4m3 bytes as uint8 [N, K], '<name>.scale_weight' as an fp32 tensor, or None)}."""
    def strip(k):
        for pre in _PREFIXES:
            if k.startswith(pre):
                return k[len(pre):]
        return k
    sd = {strip(k): v for k, v in state_dict.items()}
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight") and isinstance(v, torch.Tensor) and v.dtype == torch.float8_e4m3fn and v.dim() == 2:
            name = k[: -len(".weight")]
            s = sd.get(name + ".scale_weight")
            out[name] = (v.view(torch.uint8), None if s is None else s.to(torch.float32).reshape(-1))
    return out


_BLOCK_LINEARS = ("self_attn.q", "self_attn.k", "self_attn.v", "self_attn.o", "cross_attn.q", "cross_attn.k",
                  "cross_attn.v", "cross_attn.o", "ffn.0", "ffn.2")       # the order of block_fp8_linears


def attach_fp8_weights(model, fp8):
    """fp8_weights="keep": every block Linear quantize_fp8_ would convert, and whose checkpoint tensor
    was e4m3 (fp8_checkpoint_tensors), runs the file's own bytes: weight_fp8 = the bytes, weight_scale
    = its scale_weight broadcast to [N] (mode "tensor"; no scale_weight in the file: no weight_scale,
    which is the raw cast of the folded bf16 weight exactly).  The fused q|k|v / k|v e4m3 and scale
    buffers are built when every part of a fusion is fp8 (and all or none of them scaled).  Returns
    the number of Linears converted."""
    n = 0
    for bname, blk in model.named_modules():
        if not isinstance(blk, DiTBlock):
            continue
        for sub, lin in zip(_BLOCK_LINEARS, block_fp8_linears(blk)):
            ent = fp8.get(f"{bname}.{sub}")
            if ent is None or tuple(ent[0].shape) != tuple(lin.weight.shape):
                continue
            w8, s = ent
            dev = lin.weight.device
            lin.weight_fp8 = w8.to(dev).contiguous()
            if s is not None:
                if s.numel() not in (1, w8.shape[0]):
                    raise ValueError(f"{bname}.{sub}.scale_weight: {s.numel()} values for {w8.shape[0]} output channels")
                lin.weight_scale = s.to(dev).expand(w8.shape[0]).contiguous()
                lin.weight_scale_mode = "tensor" if s.numel() == 1 else "channel"
            n += 1
        for att in (blk.self_attn, blk.cross_attn):
            att._fw8 = att._fsw = None
            lins = [getattr(att, name) for name in att.fused]
            if not lins or any(getattr(l, "weight_fp8", None) is None for l in lins):
                continue
            scaled = [getattr(l, "weight_scale", None) is not None for l in lins]
            if any(scaled) and not all(scaled):
                continue                    # (the projections then run one by one)
            d = att.dim
            att._fw8 = torch.cat([l.weight_fp8 for l in lins], dim=0)
            if all(scaled):
                att._fsw = torch.cat([l.weight_scale for l in lins], dim=0)
            for i, l in enumerate(lins):
                l.weight_fp8 = att._fw8[i * d:(i + 1) * d]
                if all(scaled):
                    l.weight_scale = att._fsw[i * d:(i + 1) * d]
    return n


def _n_blocks(sd, prefix):
    ids = {int(k.split(".")[1]) for k in sd if k.startswith(prefix + ".") and k.split(".")[1].isdigit()}
    return len(ids)


def dit_config_from_shapes(sd):
    """Extension for checkpoints whose key hash the reference's table does not list (fine-tunes of
    another width, the tiny test checkpoints): the WanModel config read off the tensor shapes of the
    Wan key layout (wan_video_dit.py:272-308; head_dim 128 as every Wan2.1 model, patch 1x2x2).
    None when the layout is not a Wan DiT."""
    need = ("patch_embedding.weight", "blocks.0.ffn.0.weight", "text_embedding.0.weight",
            "time_embedding.0.weight", "head.head.weight")
    if not all(k in sd for k in need):
        return None
    pe = sd["patch_embedding.weight"]
    if tuple(pe.shape[2:]) != (1, 2, 2):
        return None
    dim = pe.shape[0]
    image = "blocks.0.cross_attn.k_img.weight" in sd
    control = {}
    if "ref_conv.weight" in sd:
        control["has_ref_conv"] = True
    if "control_adapter.conv.weight" in sd:     # Conv2d(64 in_dim_control_adapter, dim, 2, 2)
        control.update(add_control_adapter=True, in_dim_control_adapter=sd["control_adapter.conv.weight"].shape[1] // 64)
    return dict(WAN_COMMON, **control, has_image_input=image, has_image_pos_emb="img_emb.emb_pos" in sd,
                require_clip_embedding=image, dim=dim, in_dim=pe.shape[1], ffn_dim=sd["blocks.0.ffn.0.weight"].shape[0],
                num_heads=dim // 128, num_layers=_n_blocks(sd, "blocks"),
                text_dim=sd["text_embedding.0.weight"].shape[1], freq_dim=sd["time_embedding.0.weight"].shape[1],
                out_dim=sd["head.head.weight"].shape[0] // 4)


def vace_config_from_shapes(sd, num_layers):
    """The VaceWanModel config of a VACE key set outside the hash table: widths off the shapes, the
    n VACE blocks spread evenly over the main blocks (range(0, L, L // n): (0,2,..,28) for 1.3B,
    (0,5,..,35) for 14B, the two published layouts, wan_video_vace.py:98-113)."""
    pe = sd["vace_patch_embedding.weight"]
    dim, n = pe.shape[0], _n_blocks(sd, "vace_blocks")
    step = max(1, num_layers // n) if num_layers else 2
    return dict(vace_layers=tuple(range(0, n * step, step)), vace_in_dim=pe.shape[1], patch_size=(1, 2, 2),
                dim=dim, num_heads=dim // 128, ffn_dim=sd["vace_blocks.0.ffn.0.weight"].shape[0], eps=1e-6)


def build_dit(state_dict, device):
    sd = {k: v for k, v in state_dict.items() if not k.startswith("vace")}
    h = hash_state_dict_keys(sd)
    tables = (WAN_DIT_CONFIGS, WAN_I2V_DIT_CONFIGS, WAN_TI2V_DIT_CONFIGS, WAN_FUN_DIT_CONFIGS)
    if any(h in t for t in tables):
        cfg = dict(WAN_COMMON, **next(t[h] for t in tables if h in t))
    else:
        cfg = dit_config_from_shapes(sd)
        if cfg is None:
            return None
    model = WanModel(device=device, **cfg)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    return model


def split_animate(state_dict):
    """(the state dict without the animate adapter's keys, the adapter's keys): the two from_civitai filters of
    the reference (wan_video_dit.py:508, wan_video_animate_adapter.py:664-669).  A file without such keys
    gives (state_dict, {})."""
    ad = {k: v for k, v in state_dict.items() if isinstance(k, str) and k.startswith(ANIMATE_PREFIXES)}
    if not ad:
        return state_dict, {}
    return {k: v for k, v in state_dict.items() if k not in ad}, ad


def build_animate_adapter(adapter_sd, dit, device):
    """WanAnimateAdapter of the DiT's (dim, num_heads, num_layers) from the adapter keys of a file; the face
    encoder's in_dim off conv1_local's shape.  The motion_encoder.* tensors stay on the module unconverted."""
    need = ("pose_patch_embedding.weight", "face_encoder.conv1_local.conv.weight",
            "face_adapter.fuser_blocks.0.linear1_q.weight")
    if not all(k in adapter_sd for k in need):
        raise ValueError("animate adapter keys without pose_patch_embedding / face_encoder / face_adapter tensors")
    dim = adapter_sd["pose_patch_embedding.weight"].shape[0]
    n = _n_blocks({k[len("face_adapter."):]: v for k, v in adapter_sd.items() if k.startswith("face_adapter.")},
                  "fuser_blocks")
    L = len(dit.blocks)
    if dim != dit.dim or n != -(-L // 5):
        raise ValueError(f"the animate adapter (dim {dim}, {n} fuser blocks) does not fit the DiT (dim {dit.dim}, "
                         f"{L} blocks: {-(-L // 5)} fuser blocks)")
    model = WanAnimateAdapter(dim=dim, num_heads=dit.num_heads, num_layers=L,
                              in_dim=adapter_sd["face_encoder.conv1_local.conv.weight"].shape[1], device=device)
    model.load_state_dict({k: (v if k.startswith("motion_encoder.") else v.to(torch.bfloat16))
                           for k, v in adapter_sd.items()}, strict=True)
    return model


def build_vace(state_dict, device, num_layers=None):
    sd = {k: v for k, v in state_dict.items() if k.startswith("vace")}
    if not sd:
        return None
    h = hash_state_dict_keys(sd)
    if h == VACE_14B_HASH:
        cfg = VACE_14B
    elif sd["vace_patch_embedding.weight"].shape[0] == VACE_DEFAULT["dim"] and \
            _n_blocks(sd, "vace_blocks") == len(VACE_DEFAULT["vace_layers"]):
        cfg = VACE_DEFAULT
    else:
        if not num_layers:
            # the main-block count fixes the injection spacing; without the DiT it is known only for
            # the two published widths (wan_video_dit.py:509-536: 1536 -> 30 blocks, 5120 -> 40)
            num_layers = MAIN_LAYERS_BY_DIM.get(sd["vace_patch_embedding.weight"].shape[0])
            if not num_layers:
                raise ValueError("VACE module of an unlisted layout and width: load it together with its DiT "
                                 "so the injection layers follow the DiT's block count")
        cfg = vace_config_from_shapes(sd, num_layers)
    model = VaceWanModel(device=device, **cfg)
    model.load_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, strict=True)
    return model


# configs/model_config.py:163-164 -- the two Wan2.1 VAE file layouts (WanVideoVAE, z_dim 16)
WAN_VAE_HASHES = ("1378ea763357eea97acdef78e65d6d96", "ccc42284ea13e1ad04693284c7a09be6")


WAN22_VAE_HASH = "e1de6c02cdac79f8b739f4d3698cd216"   # the Wan2.2 VAE of TI2V-5B (WanVideoVAE38, z_dim 48)


def build_vae(state_dict, device):
    """WanVideoVAE (wan_video_vae.py:1058), or WanVideoVAE38 (:1354) for the Wan2.2 layout (its hash, or a
    48-row conv2), from the civitai layout (optionally under 'model_state')."""
    sd = state_dict.get("model_state", state_dict)
    h = hash_state_dict_keys(sd)
    if h not in WAN_VAE_HASHES + (WAN22_VAE_HASH,) and \
            not ("encoder.conv1.weight" in sd and "decoder.head.2.weight" in sd and "conv2.weight" in sd):
        return None
    from .vae import WanVideoVAE, WanVideoVAE38
    z_dim = sd["conv2.weight"].shape[0]
    if h == WAN22_VAE_HASH or z_dim == 48:
        return WanVideoVAE38(z_dim=z_dim, dim=sd["encoder.conv1.weight"].shape[0],
                             dec_dim=sd["decoder.head.2.weight"].shape[1], device=device).load_state_dict(sd)
    if z_dim != 16:
        return None
    return WanVideoVAE(z_dim=z_dim, dim=sd["encoder.conv1.weight"].shape[0], device=device).load_state_dict(sd)


T5_HASH = "9c8818c2cbea55eca56c7b447df170da"   # configs/model_config.py:161 (WanTextEncoder)


def t5_config_from_shapes(sd):
    """The WanTextEncoder config of a UMT5 key set the hash table does not list (other widths, the
    tiny test checkpoints), read off the shapes of wan_video_text_encoder.py:209-252's layout
    (shared_pos=False, head_dim 64).  None when the layout is not that encoder's."""
    need = ("token_embedding.weight", "norm.weight", "blocks.0.attn.q.weight", "blocks.0.ffn.fc1.weight",
            "blocks.0.pos_embedding.embedding.weight")
    if not all(k in sd for k in need):
        return None
    vocab, dim = sd["token_embedding.weight"].shape
    dim_attn = sd["blocks.0.attn.q.weight"].shape[0]
    num_buckets, num_heads = sd["blocks.0.pos_embedding.embedding.weight"].shape
    if dim_attn != 64 * num_heads:
        return None
    return dict(vocab=vocab, dim=dim, dim_attn=dim_attn, dim_ffn=sd["blocks.0.ffn.fc1.weight"].shape[0],
                num_heads=num_heads, num_layers=_n_blocks(sd, "blocks"), num_buckets=num_buckets)


def build_text_encoder(state_dict, device):
    if hash_state_dict_keys(state_dict) == T5_HASH:
        cfg = {}
    else:
        cfg = t5_config_from_shapes(state_dict)
        if cfg is None:
            return None
    from .t5 import WanTextEncoder
    return WanTextEncoder(device=device, **cfg).load_state_dict(state_dict)


CLIP_HASH = "5941c53e207d62f20f9025686193c40b"   # configs/model_config.py:162 (WanImageEncoder)


def build_image_encoder(state_dict, device):
    """WanImageEncoder (vstyler.clip) from models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth: the
    reference's key hash gives the ViT-H/14 defaults; any other key set that holds the visual tower
    (visual.transformer.0.attn.to_qkv.weight, with or without the "model." prefix: other widths, the tiny
    test checkpoints) gets its config from the shapes.  None when the layout is not that tower's."""
    from .clip import WanImageEncoder, config_from_shapes
    if hash_state_dict_keys(state_dict) == CLIP_HASH:
        cfg = {}
    else:
        sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in state_dict.items()
              if isinstance(k, str)}
        if "visual.transformer.0.attn.to_qkv.weight" not in sd:
            return None
        cfg = config_from_shapes(sd)
        if cfg is None:
            return None
    return WanImageEncoder(device=device, **cfg).load_state_dict(state_dict, strict=False)


def _check_experts(dits):
    """The two experts of one pipeline share the Workspace and every launch shape."""
    if len(dits) == 2:
        for name in ("dim", "num_heads", "num_layers"):
            a, b = (len(d.blocks) if name == "num_layers" else getattr(d, name) for d in dits)
            if a != b:
                raise ValueError(f"the two DiT experts differ in {name}: {a} vs {b}")


def load_models(paths, device="cuda", fp8_weights="fold"):
    """Returns {'wan_video_dit': WanModel, 'wan_video_vace': VaceWanModel, ...} for the files given
    ('wan_video_vae', 'wan_video_text_encoder' and 'wan_video_image_encoder' for those checkpoints;
    'wan_video_animate_adapter' for a DiT file that also carries pose_patch_embedding. / face_adapter. /
    face_encoder. / motion_encoder. keys, split off before the DiT's hash is taken).
    fp8_weights: "fold" -- e4m3 tensors become bf16 weights (upcast times scale_weight: normalize_keys)
    and nothing else; "keep" -- the same bf16 model (LoRA merge, hot-load and the bf16 layers work
    unchanged), whose block Linears additionally run the file's e4m3 bytes and scales on the fp8 GEMMs
    (attach_fp8_weights) instead of a second quantisation by quantize_fp8_.  A file without e4m3
    tensors loads the same either way.

    Two experts (the Wan2.2 A14B high-noise / low-noise pair): DiTs and VACE modules are collected in
    file order, 'wan_video_dit' / 'wan_video_vace' the first and 'wan_video_dit2' / 'wan_video_vace2'
    the second of each (the reference's fetch_model(..., index=2), wan_video_new.py:381-391).  A
    combined DiT+VACE file gives one of each; VACE-module-only files pair with the DiTs in order.  A
    third DiT or VACE module, or experts whose dim, num_heads or num_layers differ, is a ValueError.
    fp8_weights="keep" attaches every file's tensors to the models built from that file."""
    if fp8_weights not in ("fold", "keep"):
        raise ValueError(f"fp8_weights must be 'fold' or 'keep', got {fp8_weights!r}")
    out = {}
    dits, vaces = [], []
    vace_only = []
    for path in paths:
        raw = load_state_dict(path, device="cpu")
        fp8 = fp8_checkpoint_tensors(raw) if fp8_weights == "keep" else {}
        sd, animate_sd = split_animate(normalize_keys(raw))
        vae = build_vae(sd, device)
        if vae is not None:
            out["wan_video_vae"] = vae
            continue
        te = build_text_encoder(sd, device)
        if te is not None:
            out["wan_video_text_encoder"] = te
            continue
        ie = build_image_encoder(sd, device)
        if ie is not None:
            out["wan_video_image_encoder"] = ie
            continue
        if sd and all(k.startswith("vace") for k in sd):
            # a VACE-module-only file (the ComfyUI workflow's WanVideoVACEModelSelect input): built
            # once every file is read, with its DiT's block count when a DiT came with it
            vace_only.append((sd, fp8))
            continue
        dit = build_dit(sd, device)
        if dit is not None:
            if len(dits) == 2:
                raise ValueError(f"{path}: a third DiT checkpoint (a pipeline holds two experts, dit and dit2)")
            dits.append(dit)
            _check_experts(dits)
            if animate_sd:
                if "wan_video_animate_adapter" in out:
                    raise ValueError(f"{path}: a second animate adapter")
                out["wan_video_animate_adapter"] = build_animate_adapter(animate_sd, dit, device)
            vace = build_vace(sd, device, num_layers=len(dit.blocks))
            if vace is not None:
                if len(vaces) == 2:
                    raise ValueError(f"{path}: a third VACE module (a pipeline holds vace and vace2)")
                vaces.append(vace)
            if fp8:
                attach_fp8_weights(dit, fp8)
                if vace is not None:
                    attach_fp8_weights(vace, fp8)
            continue
        raise NotImplementedError(f"unrecognised checkpoint {path} (hash {hash_state_dict_keys(sd)})")
    for sd, fp8 in vace_only:
        if len(vaces) == 2:
            raise ValueError("a third VACE module (a pipeline holds vace and vace2)")
        # the i-th VACE module pairs with the i-th DiT (one DiT: with that one)
        dit = dits[min(len(vaces), len(dits) - 1)] if dits else None
        vace = build_vace(sd, device, num_layers=len(dit.blocks) if dit is not None else None)
        if fp8:
            attach_fp8_weights(vace, fp8)
        vaces.append(vace)
    for name, models in (("wan_video_dit", dits), ("wan_video_vace", vaces)):
        for model, suffix in zip(models, ("", "2")):
            out[name + suffix] = model
    return out
