"""CLIP ViT-H/14 image encoder on gfx950 (replaces diffsynth/models/wan_video_image_encoder.py's
WanImageEncoder.encode_image, :852-880: the clip_feature of the Wan2.1 I2V / FLF2V / Fun-InP DiTs).

encode_image = bicubic resize to 224 + normalisation + the patch convolution's im2col in one launch
(vs_clip_preprocess), the patch embedding as a vs_gemm whose VS_EPI_RES epilogue adds pos_embedding, the
pre-norm, and 31 of the 32 pre-norm blocks (VisionTransformer.forward with use_31_block, :456-478;
AttentionBlock.forward, :323-330) on the library's kernels: vs_layernorm_modulate (affine, eps 1e-5),
vs_gemm (bias / residual epilogues), vs_attn_fwd, vs_gelu_erf (nn.GELU()'s erf form).  No torch op
touches an activation.

Attention at head width 80.  vs_attn_fwd takes heads of 128 columns, so the heads are zero-padded: at
load to_qkv's weight and bias rows are scattered into [3*H*128, dim] (head h of q / k / v at columns
h*128 .. h*128+79, the other 48 rows zero) and proj's weight columns into [dim, H*128].  The zero columns
add exact zeros to every score and give zero output columns, which proj's zero columns ignore: the result
is vs_attn_fwd's contract at width 80 (scale 1/sqrt(80)), at 1.6x the arithmetic of to_qkv, proj and the
attention.

Parameters load by the reference's state-dict names (visual.*, with or without the "model." prefix;
registry md5 5941c53e..., configs/model_config.py:162); what the forward never reads (textual.*,
log_scale, visual.post_norm.*, visual.head, the last block) is dropped.
"""
import math

import torch

from . import _lib
from . import kernels as K

BF16 = torch.bfloat16
HEAD_DIM = 80           # every CLIP ViT-H head
HEAD_PAD = 128          # the head width of vs_attn_fwd
PATCH_K = 640           # 3 * 14 * 14 = 588 im2col columns, padded to the GEMM's K % 64 == 0

_BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "attn.to_qkv.weight", "attn.to_qkv.bias", "attn.proj.weight",
                 "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight",
                 "mlp.2.bias")


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def pad_head_rows(w, num_heads, parts):
    """[parts*H*80, ...] -> [parts*H*128, ...]: row p*H*80 + h*80 + d moves to p*H*128 + h*128 + d, the
    other rows zero (to_qkv's weight and bias with parts = 3; proj's transposed weight with parts = 1)."""
    tail = tuple(w.shape[1:])
    out = torch.zeros((parts * num_heads, HEAD_PAD) + tail, dtype=w.dtype, device=w.device)
    out[:, :HEAD_DIM] = w.reshape((parts * num_heads, HEAD_DIM) + tail)
    return out.reshape((parts * num_heads * HEAD_PAD,) + tail)


def attention_d80(qkv, out, num_heads, batch, scale=None):
    """Self-attention of `batch` samples at head width 80 on the zero-padded layout: qkv [batch*s,
    3*H*128] (q | k | v thirds, head h at columns h*128 .. h*128+79 of its third, the rest zero), out
    [batch*s, H*128] with the same head layout (its pad columns come out zero).  scale: 1/sqrt(80)."""
    hp = num_heads * HEAD_PAD
    if qkv.dim() != 2 or qkv.shape[1] != 3 * hp or out.dim() != 2 or out.shape[1] != hp:
        raise ValueError(f"attention_d80: qkv {tuple(qkv.shape)} / out {tuple(out.shape)} for {num_heads} padded heads")
    if scale is None:
        scale = HEAD_DIM ** -0.5
    return K.attention(qkv[:, :hp], qkv[:, hp:2 * hp], qkv[:, 2 * hp:], out, num_heads, batch, scale=scale)


def clip_preprocess(images, tokens, image_size=224):
    """tokens [n*g*g, ld >= 640] = normalised im2col of images [n, 3, H, W] bf16 (a view with a
    contiguous last dim: any image / channel / row strides) resized to image_size (vs_clip_preprocess)."""
    if images.dtype != BF16 or not images.is_cuda or images.dim() != 4 or images.shape[1] != 3 or \
            images.stride(3) != 1:
        raise ValueError(f"images: expected a bfloat16 device tensor [n, 3, H, W] with a contiguous last dim, got "
                         f"{tuple(images.shape)} {images.dtype}")
    n, _, H, W = images.shape
    g = image_size // 14
    rows, cols, ld = K._rows(tokens, "tokens")
    if image_size % 14 or rows != n * g * g or tokens.dim() != 2 or cols < PATCH_K:
        raise ValueError(f"clip_preprocess: tokens {tuple(tokens.shape)} for {n} images of {g}x{g} patches")
    _lib.check(_lib.load().vs_clip_preprocess(images.data_ptr(), images.stride(0) if n > 1 else 0, images.stride(1),
                                              images.stride(2), tokens.data_ptr(), ld, n, H, W, image_size,
                                              _stream(images)))
    return tokens


def config_from_shapes(sd):
    """The WanImageEncoder config of a CLIP key set (keys without the "model." prefix) read off its
    shapes (VisionTransformer.__init__, wan_video_image_encoder.py:386-454); None when the layout is not
    that tower's."""
    need = ("visual.patch_embedding.weight", "visual.pos_embedding", "visual.cls_embedding",
            "visual.transformer.0.attn.to_qkv.weight", "visual.transformer.0.mlp.0.weight")
    if not all(k in sd for k in need):
        return None
    pe = sd["visual.patch_embedding.weight"]
    if pe.dim() != 4 or pe.shape[1] != 3 or pe.shape[2] != pe.shape[3]:
        return None
    dim, patch = pe.shape[0], pe.shape[2]
    grid = math.isqrt(sd["visual.pos_embedding"].shape[1] - 1)
    if grid * grid + 1 != sd["visual.pos_embedding"].shape[1] or dim % HEAD_DIM:
        return None
    layers = {int(k.split(".")[2]) for k in sd if k.startswith("visual.transformer.") and k.split(".")[2].isdigit()}
    return dict(dim=dim, num_heads=dim // HEAD_DIM, mlp_ratio=sd["visual.transformer.0.mlp.0.weight"].shape[0] // dim,
                num_layers=len(layers), image_size=grid * patch, patch_size=patch)


class WanImageEncoder:
    """WanImageEncoder (wan_video_image_encoder.py:852-880): the visual tower of
    clip_xlm_roberta_vit_h_14 (:826-849) up to its second-to-last block."""

    def __init__(self, dim=1280, num_heads=16, mlp_ratio=4, num_layers=32, image_size=224, patch_size=14, eps=1e-5,
                 device="cuda"):
        if dim % num_heads or dim // num_heads != HEAD_DIM:
            raise NotImplementedError(f"CLIP ViT head_dim 80 only (dim {dim}, {num_heads} heads)")
        if dim % 64:
            raise NotImplementedError(f"dim must be a multiple of 64, got {dim}")
        if patch_size != 14 or image_size % patch_size or image_size < patch_size:
            raise NotImplementedError(f"patch 14 on an image_size that is a multiple of it, got {patch_size} / "
                                      f"{image_size}")
        if num_layers < 2:
            raise ValueError("num_layers counts the unused last block: at least 2")
        self.dim, self.num_heads, self.mlp_ratio, self.num_layers = dim, num_heads, mlp_ratio, num_layers
        self.image_size, self.patch_size, self.eps = image_size, patch_size, eps
        self.grid = image_size // patch_size
        self.tokens = self.grid * self.grid + 1
        self.device = torch.device(device)
        self.w = {}

    # ------------------------------------------------------------------ parameters
    def state_dict_shapes(self):
        """The reference's names and shapes of what the forward reads (no "model." prefix)."""
        d, m, p = self.dim, self.dim * self.mlp_ratio, self.patch_size
        out = {"visual.patch_embedding.weight": (d, 3, p, p), "visual.cls_embedding": (1, 1, d),
               "visual.pos_embedding": (1, self.tokens, d), "visual.pre_norm.weight": (d,), "visual.pre_norm.bias": (d,)}
        shapes = {"norm1.weight": (d,), "norm1.bias": (d,), "attn.to_qkv.weight": (3 * d, d), "attn.to_qkv.bias": (3 * d,),
                  "attn.proj.weight": (d, d), "attn.proj.bias": (d,), "norm2.weight": (d,), "norm2.bias": (d,),
                  "mlp.0.weight": (m, d), "mlp.0.bias": (m,), "mlp.2.weight": (d, m), "mlp.2.bias": (d,)}
        for i in range(self.num_layers - 1):
            out.update({f"visual.transformer.{i}.{k}": shapes[k] for k in _BLOCK_PARAMS})
        return out

    def load_state_dict(self, sd, strict=True):
        """Keys with or without "model."; textual.*, log_scale, visual.post_norm.*, visual.head and block
        num_layers - 1 are dropped.  A missing or mis-shaped parameter is a KeyError / ValueError; so is,
        with strict, a key that is neither read nor one of the dropped ones."""
        sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}
        last = f"visual.transformer.{self.num_layers - 1}."
        want = self.state_dict_shapes()
        extra = [k for k in sd if k not in want and not (
            k.startswith("textual.") or k.startswith("visual.post_norm.") or k.startswith(last) or
            k in ("log_scale", "logit_bias", "visual.head") or k.startswith("visual.head."))]
        if strict and extra:
            raise KeyError(f"WanImageEncoder: unexpected keys {sorted(extra)[:4]}")
        missing = [k for k in want if k not in sd]
        if missing:
            raise KeyError(f"WanImageEncoder: missing keys {missing[:4]} ({len(missing)} in all)")
        for k, shape in want.items():
            if tuple(sd[k].shape) != tuple(shape):
                raise ValueError(f"WanImageEncoder: {k} is {tuple(sd[k].shape)}, expected {tuple(shape)}")

        def dev(t):
            return t.detach().to(device=self.device, dtype=BF16).contiguous()
        H, d = self.num_heads, self.dim
        w = {}
        patch = torch.zeros((d, PATCH_K), dtype=BF16, device=self.device)
        patch[:, :3 * self.patch_size ** 2] = dev(sd["visual.patch_embedding.weight"]).reshape(d, -1)
        w["patch"] = patch
        pos = dev(sd["visual.pos_embedding"])[0]
        # row 0 of every image: bf16(bf16(cls) + pos[0]) (the cat casts cls to the activation dtype, :462)
        w["row0"] = (dev(sd["visual.cls_embedding"]).reshape(d).float() + pos[0].float()).to(BF16)
        w["pos"] = pos[1:].contiguous()
        w["pre_norm.weight"], w["pre_norm.bias"] = dev(sd["visual.pre_norm.weight"]), dev(sd["visual.pre_norm.bias"])
        for i in range(self.num_layers - 1):
            p = f"visual.transformer.{i}."
            for k in ("norm1.weight", "norm1.bias", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.0.weight",
                      "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"):
                w[f"{i}.{k}"] = dev(sd[p + k])
            w[f"{i}.attn.to_qkv.weight"] = pad_head_rows(dev(sd[p + "attn.to_qkv.weight"]), H, 3)
            w[f"{i}.attn.to_qkv.bias"] = pad_head_rows(dev(sd[p + "attn.to_qkv.bias"]), H, 3)
            w[f"{i}.attn.proj.weight"] = pad_head_rows(dev(sd[p + "attn.proj.weight"]).t(), H, 1).t().contiguous()
        self.w = w
        return self

    def init_random_(self, seed=8):
        """Synthetic weights under the reference's names (bench / probes): N(0, 1/fan_in) matrices, 0.01 N
        biases, norms 1 + 0.1 N, embeddings N(0, 1/dim)."""
        g = torch.Generator().manual_seed(seed)
        sd = {}
        for name, shape in self.state_dict_shapes().items():
            if "norm" in name and name.endswith("weight"):
                t = 1.0 + 0.1 * torch.randn(shape, generator=g)
            elif name.endswith("bias"):
                t = 0.01 * torch.randn(shape, generator=g)
            elif name.endswith("embedding"):
                t = torch.randn(shape, generator=g) / math.sqrt(self.dim)
            else:
                t = torch.randn(shape, generator=g) / math.sqrt(math.prod(shape[1:]))
            sd[name] = t.to(BF16)
        return self.load_state_dict(sd)

    # ------------------------------------------------------------------ forward
    def _images(self, videos):
        """encode_image's argument as a list of bf16 device tensors [m, 3, H, W]."""
        if isinstance(videos, torch.Tensor):
            videos = [videos]
        out = []
        for u in videos:
            if not isinstance(u, torch.Tensor) or u.dim() != 4 or u.shape[1] != 3 or u.shape[0] < 1:
                raise ValueError(f"encode_image: expected [n, 3, H, W] tensors, got {tuple(getattr(u, 'shape', ()))}")
            if u.dtype not in (BF16, torch.float32):
                raise ValueError(f"encode_image: expected bfloat16 or float32 images, got {u.dtype}")
            u = u.to(self.device)
            if u.dtype == torch.float32:        # the pipeline hands the reference bf16 frames: round first
                src = u.contiguous()
                u = torch.empty(src.shape, dtype=BF16, device=self.device)
                _lib.check(_lib.load().vs_cast(src.data_ptr(), u.data_ptr(), src.numel(), 1, _stream(src)))
            elif u.stride(3) != 1:
                raise ValueError("encode_image: the images' last dim must be contiguous")
            out.append(u)
        return out

    def encode_image(self, videos):
        """videos: a list of [1, 3, H, W] tensors or one [n, 3, H, W] tensor, bf16 or fp32 in [-1, 1]
        -> [n, 257, dim] bf16: the output of block num_layers - 2."""
        if not self.w:
            raise RuntimeError("WanImageEncoder: no weights loaded")
        images = self._images(videos)
        n = sum(u.shape[0] for u in images)
        d, H, T, gg = self.dim, self.num_heads, self.tokens, self.grid * self.grid
        dev, w = self.device, self.w
        M, hp = n * T, H * HEAD_PAD

        def buf(*shape):
            return torch.empty(shape, dtype=BF16, device=dev)
        tok, x0, x, h = buf(n * gg, PATCH_K), buf(M, d), buf(M, d), buf(M, d)
        qkv, o, f = buf(M, 3 * hp), buf(M, hp), buf(M, d * self.mlp_ratio)
        lib = _lib.load()
        i = 0
        for u in images:
            clip_preprocess(u, tok[i * gg:(i + u.shape[0]) * gg], self.image_size)
            i += u.shape[0]
        for i in range(n):
            # rows 1.. of the slab: bf16(pos + bf16(conv)), the epilogue's rounding; row 0: cls + pos[0]
            K.gemm(tok[i * gg:(i + 1) * gg], w["patch"], x0[i * T + 1:(i + 1) * T], epilogue=K.VS_EPI_RES,
                   residual=w["pos"])
            _lib.check(lib.vs_vae_copy_frames(w["row0"].data_ptr(), d, x0[i * T].data_ptr(), d, 1, d, _stream(x0)))
        K.layernorm_modulate(x0, x, self.eps, weight=w["pre_norm.weight"], bias=w["pre_norm.bias"])
        for i in range(self.num_layers - 1):
            W = lambda name: w[f"{i}.{name}"]  # noqa: E731
            K.layernorm_modulate(x, h, self.eps, weight=W("norm1.weight"), bias=W("norm1.bias"))
            K.gemm(h, W("attn.to_qkv.weight"), qkv, bias=W("attn.to_qkv.bias"))
            attention_d80(qkv, o, H, n)
            K.gemm(o, W("attn.proj.weight"), x, epilogue=K.VS_EPI_RES, bias=W("attn.proj.bias"), residual=x)
            K.layernorm_modulate(x, h, self.eps, weight=W("norm2.weight"), bias=W("norm2.bias"))
            K.gemm(h, W("mlp.0.weight"), f, bias=W("mlp.0.bias"))
            K.gelu_erf(f)
            K.gemm(f, W("mlp.2.weight"), x, epilogue=K.VS_EPI_RES, bias=W("mlp.2.bias"), residual=x)
        return x.view(n, T, d)

    __call__ = encode_image
