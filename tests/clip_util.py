"""Test-side restatement of the CLIP ViT-H/14 image encoder (WanImageEncoder.encode_image,
diffsynth/models/wan_video_image_encoder.py:852-880 over VisionTransformer.forward :456-478 and
AttentionBlock.forward :323-330), composed from oracle.wan_oracle's linear / layer_norm / attention
(generic head width) and i2v_util.gelu_erf; the preprocessing in float64 with exact-rational taps and the
reference's five bf16 roundings as torch bf16 ops; and width-80 versions of gpu_util's exact-attention
inputs and float64 reference (gpu_util's are fixed at width 128).  Everything runs on CPU tensors; never
used by the product path."""
import math

import torch
import torch.nn.functional as F

import gpu_util as G
import i2v_util as I
from oracle import wan_oracle as O

BF16 = torch.bfloat16
HD = 80
PATCH = 14
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
EPS = 1e-5

# the tiny towers of the GPU tests: 4 heads of 80, MLP 1280, 3 layers of which 2 run
TINY = dict(dim=320, num_heads=4, mlp_ratio=4, num_layers=3, image_size=224, patch_size=14)
TINY17 = dict(TINY, image_size=56)
# the real widths, two blocks running
REAL2 = dict(dim=1280, num_heads=16, mlp_ratio=4, num_layers=3, image_size=224, patch_size=14)
# one block at the CLIP width i2v_util's tiny DiT embeds (its img_emb is fixed at 1280 inputs)
WIDE1 = dict(REAL2, num_layers=2)

_BLOCK = {"norm1.weight": "d", "norm1.bias": "d", "attn.to_qkv.weight": "3d,d", "attn.to_qkv.bias": "3d",
          "attn.proj.weight": "d,d", "attn.proj.bias": "d", "norm2.weight": "d", "norm2.bias": "d",
          "mlp.0.weight": "m,d", "mlp.0.bias": "m", "mlp.2.weight": "d,m", "mlp.2.bias": "d"}


def tokens_of(cfg):
    return (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1


def param_shapes(cfg, extras=True):
    """The checkpoint's key layout for cfg (VisionTransformer.__init__, :386-454; XLMRobertaCLIP :691-708):
    all num_layers blocks, post_norm, head, log_scale and (extras) a stand-in textual.* tensor -- what
    the file holds, of which the forward reads blocks 0 .. num_layers - 2 and the embeddings."""
    d, m, p = cfg["dim"], cfg["dim"] * cfg["mlp_ratio"], cfg["patch_size"]
    sym = {"d": d, "m": m, "3d": 3 * d}
    s = {"visual.patch_embedding.weight": (d, 3, p, p), "visual.cls_embedding": (1, 1, d),
         "visual.pos_embedding": (1, tokens_of(cfg), d), "visual.pre_norm.weight": (d,), "visual.pre_norm.bias": (d,)}
    for i in range(cfg["num_layers"]):
        for k, spec in _BLOCK.items():
            s[f"visual.transformer.{i}.{k}"] = tuple(sym[t] for t in spec.split(","))
    if extras:
        s.update({"visual.post_norm.weight": (d,), "visual.post_norm.bias": (d,), "visual.head": (d, 64),
                  "log_scale": (), "textual.model.norm.weight": (32,)})
    return s


def random_weights(cfg, seed=21, prefix="", extras=True):
    """Seeded bf16 weights under the reference's key names (optionally behind `prefix`, "model."), by the
    oracle's init rule (N(0, 0.02) matrices and embeddings, 0.01 N biases, norms 1 + 0.1 N), with pre_norm's
    weight and bias halved.  pre_norm sets the scale of the residual stream (the blocks add little to it), and
    with it the size of a bf16 ulp of the output: at unit variance a few of the 10^4 .. 10^5 elements pass
    |x| = 4, where one ulp is 2^-5 = 0.031 -- above the 2e-2 the floor rule allows on top of the float64
    floor, so a single last-place flip there can pass only if the floor happens to hold one too (measured
    before the halving, 17-token tower: max-abs 0.03125 = one ulp, rel-L2 1.9e-3, floor 0 / 0).  At half
    that scale every element stays below 4 and an ulp (2^-6) is within the allowance; relative errors, which
    the rule's other clause bounds, are unchanged."""
    gen = torch.Generator("cpu").manual_seed(seed)
    W = {k: O.init_weight(k, s, gen, cfg["dim"]) for k, s in param_shapes(cfg, extras).items()}
    for k in ("visual.pre_norm.weight", "visual.pre_norm.bias"):
        W[k] = (0.5 * W[k].float()).to(BF16)
    return {prefix + k: v for k, v in W.items()}


# -------------------------------------------------------------------------------------- preprocessing
def cubic_matrix(n_in, size):
    """[size, n_in] float64: row o holds the four cubic-convolution weights (A = -0.75) of output o at
    source coordinate ((2o+1) n_in - size) / (2 size) -- floor and remainder in integers, the fraction one
    float64 division -- on tap indices clamped to the border (coinciding taps add up)."""
    o = torch.arange(size, dtype=torch.int64)
    num, den = (2 * o + 1) * n_in - size, 2 * size
    fl = torch.div(num, den, rounding_mode="floor")
    t = (num - fl * den).double() / den
    A = -0.75
    near = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1            # noqa: E731  |x| <= 1
    far = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A       # noqa: E731  1 < |x| < 2
    w = torch.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], dim=1)
    idx = torch.clamp(fl.unsqueeze(1) - 1 + torch.arange(4), 0, n_in - 1)
    return torch.zeros(size, n_in, dtype=torch.float64).scatter_add_(1, idx, w)


def interp64(u, size=224):
    """The bicubic resize of u [n, 3, H, W] (bf16 or fp32) to size x size in float64."""
    return cubic_matrix(u.shape[2], size) @ u.double().cpu() @ cubic_matrix(u.shape[3], size).t()


def rest(r):
    """The reference's five roundings on the interpolated value r [n, 3, S, S] (any float dtype), each a
    torch bf16 tensor op (:874 with torchvision's Normalize, which builds mean / std in the tensor's
    dtype): bf16(r), bf16(0.5 .), bf16(. + 0.5), bf16(. - bf16(mean)), bf16(. / bf16(std)).  Monotone."""
    x = r.to(BF16).mul(0.5).add_(0.5)
    mean = torch.as_tensor(MEAN, dtype=BF16).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=BF16).view(-1, 1, 1)
    return x.sub_(mean).div_(std)


def preprocess(u, size=224):
    """encode_image's preprocessing of u [n, 3, H, W] -> [n, 3, size, size] bf16."""
    return rest(interp64(u, size))


def preprocess_torch(u, size=224):
    """The same through torch's own F.interpolate (bf16 input: fp32 arithmetic, one rounding)."""
    return rest(F.interpolate(u, size=(size, size), mode="bicubic", align_corners=False))


def im2col(xn):
    """[n, 3, S, S] -> [n*g*g, 588]: column c*196 + ky*14 + kx of row i*g*g + py*g + px is pixel
    (c, 14 py + ky, 14 px + kx) -- Conv2d(3, dim, 14, 14)'s patches in its weight's (c, ky, kx) order."""
    n, c, S, _ = xn.shape
    g = S // PATCH
    return xn.view(n, c, g, PATCH, g, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, c * PATCH * PATCH)


def exact_image(n, H, W, seed):
    """n images [n, 3, H, W] bf16 of pixel values k / 64, k in -64..64: at source sizes 224 m (t = 0 or
    1/2, weights 1 or -3/32, 19/32) every product and partial sum of the 16 taps is exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-64, 65, (n, 3, H, W), generator=g).float() / 64).to(BF16)


EXACT_SIZES = [(448, 448), (224, 224), (448, 896)]
INTERVAL_SIZES = [(480, 832), (720, 1280), (64, 96), (225, 223), (17, 23)]
DELTA = 2.0 ** -18          # first-order fp32 error of the 16 taps, sum |w| ~ 1.4 per axis, |pixel| <= 1
MAX_WIDE = 0.005            # share of elements whose interval holds more than one bf16 value


def u8_image(H, W, seed):
    """A seeded (1, H, W, 3) uint8 image (smooth ramps + noise, so neighbouring taps differ)."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, H).view(H, 1, 1)
    xx = torch.linspace(0, 1, W).view(1, W, 1)
    base = 128 + 90 * torch.sin(6.0 * yy + torch.tensor([0.0, 1.0, 2.0])) * torch.cos(5.0 * xx)
    return (base + 30 * torch.randn(H, W, 3, generator=g)).clamp(0, 255).to(torch.uint8)[None]


def frame_of_u8(u8):
    """BasePipeline.preprocess_video of one uint8 frame on the CPU -> [1, 3, H, W] bf16 in [-1, 1]
    (oracle.wan_vae_oracle.preprocess_video's rounding points)."""
    from oracle import wan_vae_oracle as V
    return V.preprocess_video(u8)[:, :, 0].contiguous()


def interval(u, size=224):
    """(lo, hi) = (rest(r - delta), rest(r + delta)) around the float64 interpolation r of u."""
    r = interp64(u, size)
    return rest(r - DELTA), rest(r + DELTA)


# ---------------------------------------------------------------------------------------------- tower
def block(x, W, p, num_heads):
    """AttentionBlock.forward, pre-norm (:323-330): x + proj(attn(to_qkv(norm1 x))), x + fc2(gelu(fc1(norm2
    x))); attention = F.scaled_dot_product_attention at 1/sqrt(80) (flash_attention's compatibility mode)."""
    h = O.layer_norm(x, EPS, W[p + "norm1.weight"], W[p + "norm1.bias"])
    q, k, v = O.linear(h, W[p + "attn.to_qkv.weight"], W[p + "attn.to_qkv.bias"]).chunk(3, dim=-1)
    a = O.attention(q.contiguous(), k.contiguous(), v.contiguous(), num_heads)
    x = O.add(x, O.linear(a, W[p + "attn.proj.weight"], W[p + "attn.proj.bias"]))
    h = O.layer_norm(x, EPS, W[p + "norm2.weight"], W[p + "norm2.bias"])
    f = O.linear(I.gelu_erf(O.linear(h, W[p + "mlp.0.weight"], W[p + "mlp.0.bias"])), W[p + "mlp.2.weight"],
                 W[p + "mlp.2.bias"])
    return O.add(x, f)


def visual(xn, W, cfg):
    """VisionTransformer.forward(use_31_block=True) (:456-478) of the normalised images xn [n, 3, S, S]
    bf16: patch conv (no bias), cls in front, + pos_embedding, pre_norm, blocks 0 .. num_layers - 2."""
    n, d = xn.shape[0], cfg["dim"]
    x = O.linear(im2col(xn), W["visual.patch_embedding.weight"].reshape(d, -1)).view(n, -1, d)
    x = torch.cat([W["visual.cls_embedding"].to(BF16).expand(n, -1, -1), x], dim=1)
    x = O.add(x, W["visual.pos_embedding"])
    x = O.layer_norm(x, EPS, W["visual.pre_norm.weight"], W["visual.pre_norm.bias"])
    for i in range(cfg["num_layers"] - 1):
        x = block(x, W, f"visual.transformer.{i}.", cfg["num_heads"])
    return x


def encode_image(videos, W, cfg):
    """WanImageEncoder.encode_image (:864-880) of a list of [1, 3, H, W] bf16 tensors -> [n, tokens, dim]."""
    xn = torch.cat([preprocess(u, cfg["image_size"]) for u in videos])
    return visual(xn, W, cfg)


def encode_image64(videos, W, cfg):
    """The floor restatement: the same with linear / attention accumulating in float64."""
    return I.with_float64(lambda: encode_image(videos, W, cfg))


def build(cfg, W, device="cuda"):
    from vstyler.clip import WanImageEncoder
    return WanImageEncoder(device=device, **cfg).load_state_dict(W)


def sample_images(n, H, W, seed):
    """n seeded frames [1, 3, H, W] bf16 in [-1, 1] as the pipeline hands them to the encoder."""
    return [frame_of_u8(u8_image(H, W, seed + i)) for i in range(n)]


# --------------------------------------------------------------------------- attention at head width 80
def attn80_exact_inputs(B, S, H, seed):
    """gpu_util.attn_exact_inputs at head width 80, self-attention: q, k, v [B*S, H*80] bf16.  q: per
    (row, head) a 1 at a seeded column 0..78 and a seeded integer r in -2..2 at column 79; k: columns 0..78
    seeded integers -lev, lev 0..3, column 79 = 1 (every score an integer); v: zero except where
    (key + column + 3 head) % 8 == 0, there seeded integers 1..4."""
    g = torch.Generator().manual_seed(seed)
    col = torch.randint(0, HD - 1, (B * S, H), generator=g)
    r = torch.randint(-2, 3, (B * S, H), generator=g)
    q = torch.zeros(B * S, H, HD)
    q.scatter_(2, col.unsqueeze(-1), 1.0)
    q[:, :, HD - 1] = r.float()
    k = -torch.randint(0, 4, (B * S, H, HD), generator=g).float()
    k[:, :, HD - 1] = 1.0
    val = torch.randint(1, 5, (B * S, H, HD), generator=g).float()
    j = torch.arange(S).repeat(B).view(-1, 1, 1)
    h = torch.arange(H).view(1, -1, 1)
    d = torch.arange(HD).view(1, 1, -1)
    v = torch.where((j + d + 3 * h) % 8 == 0, val, torch.zeros(()))
    flat = lambda t: t.reshape(t.shape[0], H * HD).to(BF16)  # noqa: E731
    return flat(q), flat(k), flat(v)


def attn80_random_inputs(B, S, H, seed):
    """q ~ 2 N(0, 1), k, v ~ N(0, 1) as bf16 [B*S, H*80]."""
    g = torch.Generator().manual_seed(seed)
    D = H * HD
    return ((2.0 * torch.randn(B * S, D, generator=g)).to(BF16), torch.randn(B * S, D, generator=g).to(BF16),
            torch.randn(B * S, D, generator=g).to(BF16))


def attn80_ref64(q, k, v, H, B, scale, exact=False):
    """gpu_util.attn_ref64's contract at head width 80 (self-attention, [B*S, H*80] rows), float64:
    S = bf16(q c) . k with c = fp32(scale) * 1.4426950408889634f, p = exp2(S - m), o = sum p v / l,
    A = sum p |v| / l; l, smin, smax per (row, head).  exact=True also evaluates the exact problem's
    preconditions (pre-scaling leaves q unchanged; integer scores; every partial sum, up to 63 padded keys
    of weight 1 included, a whole number of the row's smallest p below 2^24 of them) into `pre`."""
    S = q.shape[0] // B
    D = H * HD
    qs = G.attn_prescale(q[:, :D], scale)
    pre = {"q_unchanged": G.same_bits(qs, q[:, :D].contiguous()), "integer": True, "exact": True, "pv_max": 0.0}
    out = {n: torch.empty(B * S, D, dtype=torch.float64) for n in ("o", "A")}
    out.update({n: torch.empty(B * S, H, dtype=torch.float64) for n in ("l", "smin", "smax")})
    for b in range(B):
        rs = slice(b * S, (b + 1) * S)
        for h in range(H):
            cs = slice(h * HD, (h + 1) * HD)
            k64, v64 = k[rs, cs].double(), v[rs, cs].double()
            s = qs[rs, cs].double() @ k64.t()
            m = s.max(dim=1, keepdim=True).values
            p = torch.exp2(s - m)
            lr = p.sum(dim=1, keepdim=True)
            pav = p @ v64.abs()
            out["o"][rs, cs] = (p @ v64) / lr
            out["A"][rs, cs] = pav / lr
            out["l"][rs, h] = (lr * torch.exp2(m)).squeeze(1)
            out["smax"][rs, h] = m.squeeze(1)
            smin = s.min(dim=1, keepdim=True).values
            out["smin"][rs, h] = smin.squeeze(1)
            if exact:
                pre["integer"] = pre["integer"] and bool((s == s.round()).all())
                units = (pav.max(dim=1, keepdim=True).values * torch.exp2(m) + 64.0) * torch.exp2(-smin)
                pre["exact"] = pre["exact"] and bool((units < 2.0 ** 24).all())
                pre["pv_max"] = max(pre["pv_max"], (pav * torch.exp2(m)).max().item())
    out["pre"] = pre
    return out


def attn80_exact_ref(q, k, v, H, B, window=G.ATTN_WINDOW):
    """(ref bf16, ambiguous bool, ref64 dict) of the exact problem at scale float32(ln 2)."""
    r = attn80_ref64(q, k, v, H, B, G.ATTN_EXACT_SCALE, exact=True)
    return r["o"].float().to(BF16), G.near_bf16_midpoint(r["o"], window), r


def pad_heads(t, H):
    """[rows, H*80] -> [rows, H*128]: head h at columns h*128 .. h*128+79, the other 48 zero (the layout
    the product's padded to_qkv produces)."""
    out = torch.zeros(t.shape[0], H, 128, dtype=t.dtype, device=t.device)
    out[:, :, :HD] = t.view(t.shape[0], H, HD)
    return out.view(t.shape[0], H * 128)


def unpad_heads(t, H):
    """(the 80 value columns [rows, H*80], the 48 pad columns [rows, H*48]) of a padded [rows, H*128]."""
    t = t.reshape(t.shape[0], H, 128)
    return t[:, :, :HD].reshape(t.shape[0], H * HD), t[:, :, HD:].reshape(t.shape[0], H * (128 - HD))


ATTN80_S = 257
