"""Test helpers for the Wan2.2 VAE (WanVideoVAE38: 48 latent channels, stride 16): a torch-CPU
*whole-sequence* restatement of its encode and decode -- the formulation the product `vstyler/vae.py` runs --
built on the primitives of oracle/wan_vae_oracle.py, plus seeded weights and a tiny configuration.

The dtype of the input selects the mode.  bf16: every operator is the oracle's (convolutions accumulate in
`wan_oracle.ACC_DTYPE`, fp32 or fp64, with one bf16 rounding; elementwise ops are torch bf16 ops), which is
what the GPU tests compare against.  float32 / float64: plain torch arithmetic in that dtype with no
rounding in between, which is what tests/golden/vae22_ref.npz -- the reference implementation's own chunked
feature-cache run in float64 (tests/golden/make_vae22_ref.py) -- is compared with.  Never used by the
product path.

Frame pairing of the whole-sequence form: the main path is the Wan2.1 one (vae_util.py); a temporal
AvgDown3D shortcut averages frames (2j-1, 2j) with a zero frame -1; a temporal DupUp3D shortcut gives latent
frame 0 one output frame (its second copy) and every later frame two."""
import math

import torch
import torch.nn.functional as F

from oracle import wan_vae_oracle as V

BF16 = torch.bfloat16

TINY_VAE22 = dict(dim=32, dec_dim=32, z_dim=48, dim_mult=(1, 2, 4, 4), num_res_blocks=2,
                  temperal_downsample=(False, True, True))
REAL_VAE22 = dict(TINY_VAE22, dim=160, dec_dim=256)

# the latent statistics of WanVideoVAE38
MEAN = [-0.2289, -0.0052, -0.1323, -0.2339, -0.2799, 0.0174, 0.1838, 0.1557,
        -0.1382, 0.0542, 0.2813, 0.0891, 0.1570, -0.0098, 0.0375, -0.1825,
        -0.2246, -0.1207, -0.0698, 0.5109, 0.2665, -0.2108, -0.2158, 0.2502,
        -0.2055, -0.0322, 0.1109, 0.1567, -0.0729, 0.0899, -0.2799, -0.1230,
        -0.0313, -0.1649, 0.0117, 0.0723, -0.2839, -0.2083, -0.0520, 0.3748,
        0.0152, 0.1957, 0.1433, -0.2944, 0.3573, -0.0548, -0.1681, -0.0667]
STD = [0.4765, 1.0364, 0.4514, 1.1677, 0.5313, 0.4990, 0.4818, 0.5013,
       0.8158, 1.0344, 0.5894, 1.0901, 0.6885, 0.6165, 0.8454, 0.4978,
       0.5759, 0.3523, 0.7135, 0.6804, 0.5833, 1.4146, 0.8986, 0.5659,
       0.7069, 0.5338, 0.4889, 0.4917, 0.4069, 0.4999, 0.6866, 0.4093,
       0.5709, 0.6065, 0.6415, 0.4944, 0.5726, 1.2042, 0.5458, 1.6887,
       0.3971, 1.0600, 0.3943, 0.5537, 0.5444, 0.4089, 0.7468, 0.7744]


# ------------------------------------------------------------------------------------------
# layout
# ------------------------------------------------------------------------------------------
def blocks(cfg, part):
    """[(main-path layers (kind, prefix, args), shortcut (c_in, c_out, ft, fs) or None)] of the four
    Down_ResidualBlocks (part "encoder") or Up_ResidualBlocks ("decoder")."""
    mult, nrb, tds = tuple(cfg["dim_mult"]), cfg["num_res_blocks"], tuple(cfg["temperal_downsample"])
    if part == "encoder":
        dims, flags, nres, sub, word = [cfg["dim"] * u for u in (1,) + mult], tds, nrb, "downsamples", "down"
    else:
        dims = [cfg["dec_dim"] * u for u in (mult[-1],) + mult[::-1]]
        flags, nres, sub, word = tds[::-1], nrb + 1, "upsamples", "up"
    out = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        p = f"{part}.{sub}.{i}.{sub}."
        last = i == len(mult) - 1
        temporal = i < len(flags) and flags[i]
        layers = [("res", f"{p}{k}.", (a if k == 0 else b, b)) for k in range(nres)]
        if not last:
            layers.append(("resample", f"{p}{nres}.", (b, f"{word}sample{'3d' if temporal else '2d'}")))
        sc = (a, b, 2 if temporal else 1, 1 if last else 2)
        out.append((layers, None if part == "decoder" and last else sc))
    return out, dims


def _resample_shapes(p, c, mode, d):
    d[p + "resample.1.weight"], d[p + "resample.1.bias"] = (c, c, 3, 3), (c,)       # the width is kept
    if mode.endswith("3d"):
        ct = 2 * c if mode == "upsample3d" else c
        d[p + "time_conv.weight"], d[p + "time_conv.bias"] = (ct, c, 3, 1, 1), (ct,)


def vae22_param_shapes(cfg=REAL_VAE22):
    """State-dict layout of the Wan2.2 VAE file (keys without the 'model.' prefix)."""
    z, d = cfg["z_dim"], {}

    def add(bl):
        for layers, _ in bl:
            for kind, p, args in layers:
                V._res_shapes(p, *args, d) if kind == "res" else _resample_shapes(p, *args, d)

    enc, ed = blocks(cfg, "encoder")
    d["encoder.conv1.weight"], d["encoder.conv1.bias"] = (ed[0], 12, 3, 3, 3), (ed[0],)
    add(enc)
    V._res_shapes("encoder.middle.0.", ed[-1], ed[-1], d)
    V._attn_shapes("encoder.middle.1.", ed[-1], d)
    V._res_shapes("encoder.middle.2.", ed[-1], ed[-1], d)
    d["encoder.head.0.gamma"] = (ed[-1], 1, 1, 1)
    d["encoder.head.2.weight"], d["encoder.head.2.bias"] = (2 * z, ed[-1], 3, 3, 3), (2 * z,)
    d["conv1.weight"], d["conv1.bias"] = (2 * z, 2 * z, 1, 1, 1), (2 * z,)
    d["conv2.weight"], d["conv2.bias"] = (z, z, 1, 1, 1), (z,)
    dec, dd = blocks(cfg, "decoder")
    d["decoder.conv1.weight"], d["decoder.conv1.bias"] = (dd[0], z, 3, 3, 3), (dd[0],)
    V._res_shapes("decoder.middle.0.", dd[0], dd[0], d)
    V._attn_shapes("decoder.middle.1.", dd[0], d)
    V._res_shapes("decoder.middle.2.", dd[0], dd[0], d)
    add(dec)
    d["decoder.head.0.gamma"] = (dd[-1], 1, 1, 1)
    d["decoder.head.2.weight"], d["decoder.head.2.bias"] = (12, dd[-1], 3, 3, 3), (12,)
    return d


def random_vae22_weights(cfg=TINY_VAE22, seed=6, prefixes=None):
    """Synthetic weights as random_vae_weights makes them: conv weights N(0, 1/fan_in), biases 0.01*N,
    gammas 1 + 0.1*N; all bf16.  prefixes: only the tensors whose names start with one of them (a single
    block of the real configuration, whose 705 M parameters no test needs at once)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in vae22_param_shapes(cfg).items():
        if prefixes is not None and not name.startswith(tuple(prefixes)):
            continue
        if name.endswith("gamma"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith("bias"):
            t = 0.01 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(math.prod(shape[1:]))
        out[name] = t.to(BF16)
    return out


# ------------------------------------------------------------------------------------------
# operators: the oracle's on bf16, plain arithmetic in the input's dtype otherwise
# ------------------------------------------------------------------------------------------
def _cconv(x, w, b, padding, stride=1):
    if x.dtype == BF16:
        return V.causal_conv3d(x, w, b, padding, stride=stride)
    pt, ph, pw = padding
    return F.conv3d(F.pad(x, (pw, pw, ph, ph, 2 * pt, 0)), w.to(x.dtype), b.to(x.dtype), stride=stride)


def _conv2d(x, w, b, stride=1, padding=0):
    if x.dtype == BF16:
        return V.conv2d(x, w, b, stride=stride, padding=padding)
    return F.conv2d(x, w.to(x.dtype), b.to(x.dtype), stride=stride, padding=padding)


def _norm(x, gamma):
    return V.rms_norm(x, gamma.to(x.dtype))


def _conv3(x, W, p):
    return _cconv(x, W[p + "weight"], W[p + "bias"], (1, 1, 1))


def res_block(x, W, p):
    h = _cconv(x, W[p + "shortcut.weight"], W[p + "shortcut.bias"], (0, 0, 0)) if p + "shortcut.weight" in W else x
    x = _conv3(F.silu(_norm(x, W[p + "residual.0.gamma"])), W, p + "residual.2.")
    return _conv3(F.silu(_norm(x, W[p + "residual.3.gamma"])), W, p + "residual.6.") + h


def attn_block(x, W, p):
    if x.dtype == BF16:
        return V.attention_block(x, W, p)
    b, c, t, h, w = x.shape
    y = _norm(x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w), W[p + "norm.gamma"])
    q, k, v = _conv2d(y, W[p + "to_qkv.weight"], W[p + "to_qkv.bias"]).reshape(b * t, 3 * c, h * w).transpose(1, 2) \
        .chunk(3, dim=-1)
    o = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(c), dim=-1) @ v
    o = _conv2d(o.transpose(1, 2).reshape(b * t, c, h, w), W[p + "proj.weight"], W[p + "proj.bias"])
    return o.reshape(b, t, c, h, w).permute(0, 2, 1, 3, 4) + x


def _up2(x):
    """Upsample.forward: nearest-exact x2 computed in fp32 and cast back (exact for bf16 and fp32; a float64
    run is rounded to fp32 here, as the reference's is)."""
    return x.float().repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1).type_as(x)


def resample(x, W, p, mode):
    """Resample38 over the whole sequence: frame 0 passes through both time convs; the upsample time conv
    runs over frames 1.., the downsample one over windows (2j-2, 2j-1, 2j)."""
    b, c, t, h, w = x.shape
    if mode == "upsample3d" and t > 1:
        y = _cconv(x[:, :, 1:], W[p + "time_conv.weight"], W[p + "time_conv.bias"], (1, 0, 0))
        y = y.reshape(b, 2, c, t - 1, h, w)
        x = torch.cat([x[:, :, :1], torch.stack((y[:, 0], y[:, 1]), 3).reshape(b, c, 2 * (t - 1), h, w)], 2)
    t = x.shape[2]
    x2 = x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
    if mode.startswith("up"):
        x2 = _conv2d(_up2(x2), W[p + "resample.1.weight"], W[p + "resample.1.bias"], padding=1)
    else:
        x2 = _conv2d(F.pad(x2, (0, 1, 0, 1)), W[p + "resample.1.weight"], W[p + "resample.1.bias"], stride=2)
    x = x2.reshape(b, t, *x2.shape[1:]).permute(0, 2, 1, 3, 4)
    if mode == "downsample3d" and t > 1:
        y = _cconv(x, W[p + "time_conv.weight"], W[p + "time_conv.bias"], (0, 0, 0), stride=(2, 1, 1))
        x = torch.cat([x[:, :, :1], y], 2)
    return x


def avg_down(x, c_out, ft, fs):
    """AvgDown3D over the whole sequence: (ft, fs, fs) blocks folded into the channels, means over
    groups of c_in ft fs fs / c_out of them; ft 2 pairs frames (2j-1, 2j), frame -1 zero."""
    if ft == 2:
        x = F.pad(x, (0, 0, 0, 0, 1, 0))
    b, c, t, h, w = x.shape
    x = x.reshape(b, c, t // ft, ft, h // fs, fs, w // fs, fs).permute(0, 1, 3, 5, 7, 2, 4, 6)
    return x.reshape(b, c_out, c * ft * fs * fs // c_out, t // ft, h // fs, w // fs).mean(dim=2)


def dup_up(x, c_out, ft, fs):
    """DupUp3D over the whole sequence: channels repeated c_out ft fs fs / c_in times and unfolded into
    (ft, fs, fs) blocks; the first ft - 1 output frames dropped (the reference's first_chunk)."""
    b, c, t, h, w = x.shape
    x = x.repeat_interleave(c_out * ft * fs * fs // c, dim=1).reshape(b, c_out, ft, fs, fs, t, h, w)
    return x.permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(b, c_out, t * ft, h * fs, w * fs)[:, :, ft - 1:]


def run_block(x, W, layers, sc, part):
    """One Down_ / Up_ResidualBlock: main path + parameter-free shortcut of the block's input."""
    y = x
    for kind, p, args in layers:
        y = res_block(y, W, p) if kind == "res" else resample(y, W, p, args[1])
    if sc is None:
        return y
    return y + (avg_down if part == "encoder" else dup_up)(x, sc[1], sc[2], sc[3])


def patchify(x):
    """b c f (h q) (w r) -> b (c r q) f h w with q = r = 2."""
    b, c, f, h, w = x.shape
    return x.reshape(b, c, f, h // 2, 2, w // 2, 2).permute(0, 1, 6, 4, 2, 3, 5).reshape(b, 4 * c, f, h // 2, w // 2)


def unpatchify(x):
    """b (c r q) f h w -> b c f (h q) (w r) with q = r = 2."""
    b, c, f, h, w = x.shape
    return x.reshape(b, c // 4, 2, 2, f, h, w).permute(0, 1, 4, 5, 3, 6, 2).reshape(b, c // 4, f, 2 * h, 2 * w)


def scale(z_dim, dtype):
    """(mean, 1 / std) as the model applies them in `dtype` (fp32 values, converted)."""
    mean = torch.tensor(MEAN[:z_dim]).to(dtype).view(1, z_dim, 1, 1, 1)
    inv_std = (1.0 / torch.tensor(STD[:z_dim])).to(dtype).view(1, z_dim, 1, 1, 1)
    return mean, inv_std


def encode_whole(x, W, cfg=TINY_VAE22):
    """VideoVAE38_.encode over the whole sequence; x (1, 3, T, H, W), returns the normalised mu."""
    t = 1 + 4 * ((x.shape[2] - 1) // 4)
    x = _conv3(patchify(x[:, :, :t]), W, "encoder.conv1.")
    for layers, sc in blocks(cfg, "encoder")[0]:
        x = run_block(x, W, layers, sc, "encoder")
    x = res_block(x, W, "encoder.middle.0.")
    x = attn_block(x, W, "encoder.middle.1.")
    x = res_block(x, W, "encoder.middle.2.")
    x = _conv3(F.silu(_norm(x, W["encoder.head.0.gamma"])), W, "encoder.head.2.")
    mu = _cconv(x, W["conv1.weight"], W["conv1.bias"], (0, 0, 0))[:, :cfg["z_dim"]]
    mean, inv_std = scale(cfg["z_dim"], mu.dtype)
    return (mu - mean) * inv_std


def decode_whole(z, W, cfg=TINY_VAE22):
    """VideoVAE38_.decode over the whole sequence; z (1, 48, T, h, w) -> (1, 3, 4T-3, 16h, 16w), unclamped."""
    mean, inv_std = scale(cfg["z_dim"], z.dtype)
    x = _cconv(z / inv_std + mean, W["conv2.weight"], W["conv2.bias"], (0, 0, 0))
    x = _conv3(x, W, "decoder.conv1.")
    x = res_block(x, W, "decoder.middle.0.")
    x = attn_block(x, W, "decoder.middle.1.")
    x = res_block(x, W, "decoder.middle.2.")
    for layers, sc in blocks(cfg, "decoder")[0]:
        x = run_block(x, W, layers, sc, "decoder")
    return unpatchify(_conv3(F.silu(_norm(x, W["decoder.head.0.gamma"])), W, "decoder.head.2."))


def single_decode(z, W, cfg=TINY_VAE22):
    return decode_whole(z, W, cfg).clamp_(-1, 1)


# ------------------------------------------------------------------------------------------
# tiling: WanVideoVAE's rule and blend (the oracle's task list and masks) at factor 16
# ------------------------------------------------------------------------------------------
def tiled_encode(video, W, tile_size, tile_stride, cfg=TINY_VAE22):
    f = 16
    size, stride = (tile_size[0] * f, tile_size[1] * f), (tile_stride[0] * f, tile_stride[1] * f)
    _, _, T, H, Wd = video.shape
    out_t = (T + 3) // 4
    weight = torch.zeros((1, 1, out_t, H // f, Wd // f), dtype=video.dtype)
    values = torch.zeros((1, cfg["z_dim"], out_t, H // f, Wd // f), dtype=video.dtype)
    for h, h_, w, w_ in V.tile_tasks(H, Wd, size, stride):
        hs = encode_whole(video[:, :, :, h:h_, w:w_], W, cfg)
        mask = V.build_mask(hs.shape[3], hs.shape[4], (h == 0, h_ >= H, w == 0, w_ >= Wd),
                            ((size[0] - stride[0]) // f, (size[1] - stride[1]) // f)).to(video.dtype)
        th, tw = h // f, w // f
        values[:, :, :, th:th + hs.shape[3], tw:tw + hs.shape[4]] += hs * mask
        weight[:, :, :, th:th + hs.shape[3], tw:tw + hs.shape[4]] += mask
    return values / weight


def tiled_decode(z, W, tile_size, tile_stride, cfg=TINY_VAE22):
    f = 16
    _, _, T, H, Wd = z.shape
    out_t = T * 4 - 3
    weight = torch.zeros((1, 1, out_t, H * f, Wd * f), dtype=z.dtype)
    values = torch.zeros((1, 3, out_t, H * f, Wd * f), dtype=z.dtype)
    for h, h_, w, w_ in V.tile_tasks(H, Wd, tile_size, tile_stride):
        v = decode_whole(z[:, :, :, h:h_, w:w_], W, cfg)
        mask = V.build_mask(v.shape[3], v.shape[4], (h == 0, h_ >= H, w == 0, w_ >= Wd),
                            ((tile_size[0] - tile_stride[0]) * f, (tile_size[1] - tile_stride[1]) * f)).to(z.dtype)
        values[:, :, :, h * f:h * f + v.shape[3], w * f:w * f + v.shape[4]] += v * mask
        weight[:, :, :, h * f:h * f + v.shape[3], w * f:w * f + v.shape[4]] += mask
    return (values / weight).clamp_(-1, 1)
