"""Wan2.2-Animate's motion encoder on gfx950 (replaces Generator.get_motion,
diffsynth/models/wan_video_animate_adapter.py:321-612): face frames -> one 512-vector per frame.

The model is a StyleGAN2-style encoder that the reference runs in the pipeline dtype (bf16) on every face
frame, once per call: a 1x1 stem 3 -> C, log2(size) - 2 ResBlocks down to 4x4, a 4x4 conv to 512, five
EqualLinears 512 -> ... -> 20 and Direction, a 512 x 20 QR basis.  Here every convolution is vs_vae_conv on
channels-last frames, every linear vs_gemm with the bias epilogue, and what lies between them is one pass each
(include/vstyler_motion.h): the stem, FusedLeakyReLU fused into the 4x4 blur and into the ResBlock merge, and
Direction.  One ResBlock is conv1 -> lrelu_blur -> conv2, lrelu_blur(step 2) -> skip conv, lrelu_merge: each
activation tensor is read once and written once between convolutions.
"""
import math
import re

import torch

from . import kernels as K
from .vae import ConvW, conv

BF16 = torch.bfloat16
PREFIX = "motion_encoder."
# EncoderApp.channels (:515-525)
CHANNELS = {4: 512, 8: 512, 16: 512, 32: 512, 64: 256, 128: 128, 256: 64, 512: 32, 1024: 16}
STYLE_DIM = 512
N_FC = 5
ENCODE_BS = 8           # the reference's encode_bs (after_patch_embedding, :630)


def expected_shapes(size, motion_dim=20):
    """Parameter names (without the `motion_encoder.` prefix) and shapes of Generator(size, 512, motion_dim),
    the Blur buffers aside (they hold the constant [1, 3, 3, 1] kernel, which the blur kernel has built in)."""
    log_size = int(math.log2(size))
    if 2 ** log_size != size or size < 8 or size not in CHANNELS or CHANNELS[size] % 8:
        raise ValueError(f"motion encoder: size {size} is not a power of two in 8..512")
    p = "enc.net_app.convs."
    c = CHANNELS[size]
    s = {p + "0.0.weight": (c, 3, 1, 1), p + "0.1.bias": (1, c, 1, 1)}
    n = 1
    for i in range(log_size, 2, -1):
        co = CHANNELS[2 ** (i - 1)]
        b = f"{p}{n}."
        s[b + "conv1.0.weight"], s[b + "conv1.1.bias"] = (c, c, 3, 3), (1, c, 1, 1)
        s[b + "conv2.1.weight"], s[b + "conv2.2.bias"] = (co, c, 3, 3), (1, co, 1, 1)
        s[b + "skip.1.weight"] = (co, c, 1, 1)
        c, n = co, n + 1
    s[f"{p}{n}.weight"] = (STYLE_DIM, c, 4, 4)
    for i in range(N_FC):
        o = STYLE_DIM if i < N_FC - 1 else motion_dim
        s[f"enc.fc.{i}.weight"], s[f"enc.fc.{i}.bias"] = (o, STYLE_DIM), (o,)
    s["dec.direction.weight"] = (STYLE_DIM, motion_dim)
    return s


def size_of(state_dict, prefix=PREFIX):
    """The `size` whose complete key set (with its shapes) the dict holds, or None: the number of ResBlocks
    gives it."""
    pat = re.compile(re.escape(prefix) + r"enc\.net_app\.convs\.(\d+)\.conv1\.0\.weight$")
    nb = sum(1 for k in state_dict if pat.match(k))
    size = 2 ** (nb + 2)
    d = state_dict.get(prefix + "dec.direction.weight")
    if nb < 1 or size not in CHANNELS or d is None or d.dim() != 2:
        return None
    try:
        want = expected_shapes(size, d.shape[1])
    except ValueError:
        return None
    for k, shape in want.items():
        t = state_dict.get(prefix + k)
        if t is None or tuple(t.shape) != shape:
            return None
    return size


def _scaled(w, fan_in):
    """EqualConv2d / EqualLinear's `self.weight * self.scale` on the bf16 module, with that very expression."""
    return w.detach().to(BF16) * (1 / math.sqrt(fan_in))


class MotionEncoder:
    """Generator(size, 512, motion_dim).get_motion from the `motion_encoder.*` tensors of a Wan2.2-Animate file.
    Weights are prepared once: every EqualConv2d / EqualLinear weight as (w.to(bf16) * scale), laid out
    [cout][ky][kx][cin]; biases in bf16; Direction's Q = qr((w.to(bf16) + 1e-8).float()) on the host, rounded
    to bf16 (custom_qr; the reference recomputes it on every call, the value does not change)."""

    def __init__(self, state_dict, device=None, prefix=PREFIX):
        size = size_of(state_dict, prefix)
        if size is None:
            raise NotImplementedError("motion encoder: the motion_encoder.* weights are absent or incomplete (no "
                                      "Generator(size, 512, m) key set): pass the motion vectors as animate_face_motion=")
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        dev = sd["dec.direction.weight"].device if device is None else torch.device(device)
        self.size, self.device = size, dev
        self.motion_dim = sd["dec.direction.weight"].shape[1]
        if self.motion_dim > 32:
            raise NotImplementedError("motion encoder: motion_dim above 32")
        p = "enc.net_app.convs."
        w0 = sd[p + "0.0.weight"]
        self.c0 = w0.shape[0]
        self.stem_w = _scaled(w0, 3).reshape(self.c0, 3).to(dev).contiguous()
        self.stem_b = sd[p + "0.1.bias"].detach().to(BF16).reshape(-1).to(dev).contiguous()
        self.blocks = []
        n = 1
        while p + f"{n}.conv1.0.weight" in sd:
            b = f"{p}{n}."
            w1, w2, ws = sd[b + "conv1.0.weight"], sd[b + "conv2.1.weight"], sd[b + "skip.1.weight"]
            cin = w1.shape[1]
            self.blocks.append(dict(
                cin=cin, cout=w2.shape[0],
                conv1=ConvW(_scaled(w1, cin * 9), None, dev), conv2=ConvW(_scaled(w2, cin * 9), None, dev),
                skip=ConvW(_scaled(ws, cin), None, dev),
                b1=sd[b + "conv1.1.bias"].detach().to(BF16).reshape(-1).to(dev).contiguous(),
                b2=sd[b + "conv2.2.bias"].detach().to(BF16).reshape(-1).to(dev).contiguous()))
            n += 1
        wl = sd[f"{p}{n}.weight"]
        self.last = ConvW(_scaled(wl, wl.shape[1] * 16), None, dev)
        self.fc = [(_scaled(sd[f"enc.fc.{i}.weight"], STYLE_DIM).to(dev).contiguous(),
                    (sd[f"enc.fc.{i}.bias"].detach().to(BF16) * 1).to(dev).contiguous()) for i in range(N_FC)]
        d = sd["dec.direction.weight"].detach()
        if d.is_meta:
            q = torch.empty(tuple(d.shape), dtype=BF16, device="meta")
        else:
            q = torch.linalg.qr((d.to(BF16) + 1e-8).float().cpu())[0].to(BF16)
        self.q = q.to(dev).contiguous()                             # [512, m]: out[t][j] = sum_i alpha[t][i] q[j][i]
        from .models import Workspace
        self.ws = Workspace(dev)                                    # kernels never allocate
        self._sizes = {}

    def _buf(self, role, shape):
        """A view of `shape` at the start of the flat buffer of `role`, which grows to the largest request
        (the smaller one is dropped): what the encoder keeps between calls is one chunk's working set."""
        numel = math.prod(int(s) for s in shape)
        have = self._sizes.get(role, 0)
        if have < numel:
            self.ws.bufs.pop(("motion." + role, (have,), BF16), None)
            self._sizes[role] = have = numel
        return self.ws.get("motion." + role, (have,))[:numel].view(*shape)

    def _check(self, frames):
        S = self.size
        if not isinstance(frames, torch.Tensor):
            raise ValueError("motion encoder: frames must be a tensor")
        if frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3:
            T, hw = frames.shape[0], tuple(frames.shape[1:3])
        elif frames.dtype == BF16 and frames.dim() == 4 and frames.shape[0] == 3:
            T, hw = frames.shape[1], tuple(frames.shape[2:])
        else:
            raise ValueError(f"motion encoder: frames must be uint8 [T, {S}, {S}, 3] or bfloat16 [3, T, {S}, {S}], got "
                             f"{tuple(frames.shape)} {frames.dtype}")
        if hw != (S, S) or T < 1:
            raise ValueError(f"motion encoder: face frames must be {S} x {S} (size {S}; the reference does not resize "
                             f"either), got {hw[0]} x {hw[1]}")
        return T

    def _trunk(self, chunk, n, feat):
        """The stem and the ResBlocks on n frames; the last block's output lands in feat [n, 4, 4, 512].  Six
        flat buffers serve every level (each as large as its largest use, which is level 0's): the block input
        and conv2's output alternate between `a` and `b` (the merge runs in place on conv2's output), conv1's
        output, the two blurred tensors and the skip conv's output have one each."""
        S = self.size
        x = K.motion_stem(chunk, self.stem_w, self.stem_b, self._buf("a", (n, S, S, self.c0)))
        for i, b in enumerate(self.blocks):
            H, ci, co = x.shape[1], b["cin"], b["cout"]
            h2 = H // 2
            t1 = conv(x.view(n, 1, H, H, ci), b["conv1"], (1, H, H), pad=(0, 1, 1), y=self._buf("c1", (n, 1, H, H, ci)))
            bl = K.lrelu_blur(t1.view(n, H, H, ci), self._buf("bl", (n, H + 1, H + 1, ci)), b["b1"], (2, 2), 1)
            last = i == len(self.blocks) - 1
            y2 = feat.view(n, 1, h2, h2, co) if last else self._buf("ab"[(i + 1) % 2], (n, 1, h2, h2, co))
            t2 = conv(bl.view(n, 1, H + 1, H + 1, ci), b["conv2"], (1, h2, h2), stride=(1, 2, 2), y=y2)
            bs = K.lrelu_blur(x, self._buf("bs", (n, h2, h2, ci)), None, (1, 1), 2)
            sk = conv(bs.view(n, 1, h2, h2, ci), b["skip"], (1, h2, h2), y=self._buf("sk", (n, 1, h2, h2, co)))
            x = K.lrelu_merge(t2.view(n, h2, h2, co), b["b2"], sk.view(n, h2, h2, co))
        return x

    @torch.no_grad()
    def encode(self, frames, chunk=ENCODE_BS):
        """frames uint8 [T, size, size, 3] or bf16 [3, T, size, size] -> [T, 512] bf16 on the device (a new
        tensor).  The conv trunk runs in chunks of `chunk` frames out of buffers kept by this object; the tail
        (4x4 conv, linears, Direction) once over all T rows; a ragged last chunk runs in the same buffers.  The result does not depend on the chunk size."""
        T = self._check(frames)
        if self.q.is_meta:
            raise RuntimeError("motion encoder: built on the meta device")
        frames = frames.to(self.device).contiguous()
        u8 = frames.dtype == torch.uint8
        chunk = max(1, min(int(chunk), T))
        cl = self.blocks[-1]["cout"]
        feat = self._buf("feat", (T, 4, 4, cl))
        for t0 in range(0, T, chunk):
            n = min(chunk, T - t0)
            part = frames[t0:t0 + n] if u8 else frames[:, t0:t0 + n].contiguous()
            self._trunk(part, n, feat[t0:t0 + n])
        h = conv(feat.view(T, 1, 4, 4, cl), self.last, (1, 1, 1), y=self._buf("w", (T, 1, 1, 1, STYLE_DIM)))
        h = h.view(T, STYLE_DIM)
        for i, (w, b) in enumerate(self.fc):
            o = self._buf(f"fc{i}", (T, STYLE_DIM if i < N_FC - 1 else 32))
            h = K.gemm(h, w, o[:, :w.shape[0]], bias=b)
        return K.motion_direction(h, self.q, torch.empty((T, STYLE_DIM), device=self.device, dtype=BF16))
