"""Cost of the motion encoder at the real dims (MotionEncoder size 512: stem 3 -> 32, seven ResBlocks
512^2 -> 4^2, T = 77 face frames in chunks of 8), seeded weights.

(a) encode(frames) end to end: HIP events around back-to-back calls, WINDOWS windows; median and spread.
(b) every launch of one chunk of 8 frames alone, by family and level: vs_vae_conv (conv1, conv2, skip), vs_lrelu_blur
    (in front of conv2, with ACT; in front of the skip conv, step 2), vs_lrelu_merge, the stem; and the tail
    (4x4 conv, five linears, Direction) at T rows.  ms per launch and, times the chunks, per encode.
(c) the achieved bytes/s of the three streaming kernels at the 512^2 and 256^2 levels (bytes the algorithm needs:
    each input read once, each output written once) against the copy ceiling measured in the same run: torch copy_
    of the 512^2 x 32-channel chunk (tests/probes/rowpipe/copy_ceiling.py's method).

  python tests/probes/motion_encode.py [--frames 77] [--windows 5] [--out FILE]"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "..", "video-styler_amd"), os.path.join(HERE, "..")]
import torch  # noqa: E402

import motion_util as M  # noqa: E402
from vstyler import kernels as K  # noqa: E402
from vstyler.motion import ENCODE_BS, MotionEncoder  # noqa: E402
from vstyler.vae import conv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=77)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--out", default=None, help="also write the log lines to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
BF16 = torch.bfloat16
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def timed(fn, windows=3):
    """median ms per call over `windows` windows of at least 0.2 s each, after a warm-up."""
    events(fn, 2)
    it = max(3, int(200.0 / max(events(fn, 3), 1e-3)))
    v = sorted(events(fn, it) for _ in range(windows))
    return v[len(v) // 2]


S, T, n = args.size, args.frames, ENCODE_BS
net = MotionEncoder(M.motion_weights(S, seed=41), device=dev)
g = torch.Generator(device=dev).manual_seed(3)
frames = torch.randint(0, 256, (T, S, S, 3), generator=g, device=dev, dtype=torch.uint8)
chunks = T / n
say(f"MotionEncoder size {S}, T = {T} frames, chunks of {n} ({len(net.blocks)} ResBlocks)")
events(lambda: net.encode(frames), 2)
once = events(lambda: net.encode(frames), 2)
it = max(2, int(1500.0 / once) + 1)
ms = [events(lambda: net.encode(frames), it) for _ in range(args.windows)]
v = sorted(ms)
say(f"(a) encode: median {v[len(v) // 2]:.2f} ms, spread {v[-1] - v[0]:.2f} ms, windows {[round(x, 2) for x in ms]} "
    f"({it} calls per window)")

# (c)'s ceiling first: a copy of the largest activation of a chunk
big = torch.empty((n, S, S, net.c0), device=dev, dtype=BF16).normal_()
dst = torch.empty_like(big)
ceil_ms = timed(lambda: dst.copy_(big))
ceiling = 2 * big.numel() * 2 / ceil_ms / 1e9
say(f"copy ceiling: copy_ of [{n}, {S}, {S}, {net.c0}] bf16 ({big.numel() * 2 / 1e6:.0f} MB in, same out): "
    f"{ceil_ms * 1e3:.1f} us, {ceiling:.2f} TB/s read + write")


def rnd(*shape):
    return torch.empty(shape, device=dev, dtype=BF16).normal_()


say(f"(b) launches of one chunk of {n} frames: ms per launch | per encode ({chunks:.3f} chunks)")
fam = {"stem": 0.0, "conv": 0.0, "blur": 0.0, "merge": 0.0}
out = rnd(n, S, S, net.c0)
t = timed(lambda: K.motion_stem(frames[:n], net.stem_w, net.stem_b, out))
byt = n * S * S * (3 + 2 * net.c0)
fam["stem"] += t * chunks
say(f"  stem {S}^2 3->{net.c0}: {t:.3f} | {t * chunks:.2f}   {byt / t / 1e9:.2f} TB/s ({100 * byt / t / 1e9 / ceiling:.0f} % of the ceiling)")
H = S
for i, b in enumerate(net.blocks):
    ci, co, h2 = b["cin"], b["cout"], H // 2
    x, t1, bl = rnd(n, H, H, ci), rnd(n, 1, H, H, ci), rnd(n, H + 1, H + 1, ci)
    t2, bs, sk = rnd(n, 1, h2, h2, co), rnd(n, h2, h2, ci), rnd(n, 1, h2, h2, co)
    ops = {
        "conv1": (lambda: conv(x.view(n, 1, H, H, ci), b["conv1"], (1, H, H), pad=(0, 1, 1), y=t1), 0),
        "blur+act": (lambda: K.lrelu_blur(t1.view(n, H, H, ci), bl, b["b1"], (2, 2), 1),
                     2 * n * ci * (H * H + (H + 1) ** 2)),
        "conv2": (lambda: conv(bl.view(n, 1, H + 1, H + 1, ci), b["conv2"], (1, h2, h2), stride=(1, 2, 2), y=t2), 0),
        "blur/2": (lambda: K.lrelu_blur(x, bs, None, (1, 1), 2), 2 * n * ci * (H * H + h2 * h2)),
        "skip": (lambda: conv(bs.view(n, 1, h2, h2, ci), b["skip"], (1, h2, h2), y=sk), 0),
        "merge": (lambda: K.lrelu_merge(t2.view(n, h2, h2, co), b["b2"], sk.view(n, h2, h2, co)), 3 * 2 * n * co * h2 * h2),
    }
    parts = []
    for name, (fn, byt) in ops.items():
        t = timed(fn)
        fam["conv" if byt == 0 else "merge" if name == "merge" else "blur"] += t * chunks
        parts.append(f"{name} {t:.3f}" + (f" ({byt / t / 1e9:.2f} TB/s, {100 * byt / t / 1e9 / ceiling:.0f} %)" if byt else ""))
    say(f"  level {H}^2 {ci}->{co}: " + ", ".join(parts))
    del x, t1, bl, t2, bs, sk
    H = h2
feat = rnd(T, 1, 4, 4, net.blocks[-1]["cout"])


def tail():
    h = conv(feat, net.last, (1, 1, 1), y=net._buf("w", (T, 1, 1, 1, 512))).view(T, 512)
    for i, (w, bias) in enumerate(net.fc):
        h = K.gemm(h, w, net._buf(f"fc{i}", (T, 512 if i < 4 else 32))[:, :w.shape[0]], bias=bias)
    return K.motion_direction(h, net.q, net._buf("probe.out", (T, 512)))


tt = timed(tail)
say(f"  tail at {T} rows (4x4 conv, 5 linears, Direction): {tt:.3f} ms")
say("per encode by family: " + ", ".join(f"{k} {v:.2f} ms" for k, v in fam.items()) + f", tail {tt:.2f} ms; sum "
    f"{sum(fam.values()) + tt:.2f} ms")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
