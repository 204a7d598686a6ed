"""Cost of the first-frame segment at the Wan2.2-TI2V-5B dims (dim 3072, 24 heads, ffn 14336, 48 channels),
1280x704x121 (latents 48 x 31 x 44 x 80: S = 27 280 tokens, n0 = 880 per latent frame), B = 2 (CFG), random
weights as bench.py builds them.

The whole CFG step (hipGraph replay) of the same model with fuse_vae_embedding_in_latents (two modulation
rows per sample: the _seg LayerNorms and the gated GEMMs' seg_rows epilogue, the first frame pinned after
the Euler update) against the plain step, REPS interleaved repeats, host clock around a synchronise.

  python tests/probes/ti2v_step.py [--reps 5] [--layers 30] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "video-styler_amd"))
import torch

from vstyler import kernels as K
from vstyler import model_fn_wan_video
from vstyler.flow_match import FlowMatchScheduler
from vstyler.models import WanModel, init_random_
from vstyler.pipeline import DenoiseStepper

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=30)
ap.add_argument("--out", default=None, help="also write the JSON record to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
BF16 = torch.bfloat16
D, HEADS, FFN, C = 3072, 24, 14336, 48
T, Hl, Wl = 31, 704 // 16, 1280 // 16
N0 = (Hl // 2) * (Wl // 2)
S = T * N0
B, L = 2, 512
rec = {"S": S, "n0": N0, "B": B, "reps": args.reps, "layers": args.layers}


def summary(ms):
    v = sorted(ms)
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(v[len(v) // 2], 4), "spread_ms": round(v[-1] - v[0], 4)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1000 * (time.perf_counter() - t0)


dit = init_random_(WanModel(dim=D, in_dim=C, ffn_dim=FFN, out_dim=C, text_dim=4096, freq_dim=256, eps=1e-6,
                            patch_size=(1, 2, 2), num_heads=HEADS, num_layers=args.layers, seperated_timestep=True,
                            require_clip_embedding=False, require_vae_embedding=False,
                            fuse_vae_embedding_in_latents=True, device=dev), seed=5)
g = torch.Generator().manual_seed(1)
ctx = 0.1 * torch.randn(2, L, 4096, generator=g)
ctx[0, 32:] = 0
ctx[1, 96:] = 0
ctx = ctx.to(BF16).to(dev)
first = torch.randn(1, C, 1, Hl, Wl, generator=g).to(BF16).to(dev)
n_steps = 64
sched = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
sched.set_timesteps(n_steps, shift=5.0)
ts = sched.timesteps.to(BF16).to(dev)
ds = torch.tensor([sched.delta(i) for i in range(n_steps)], dtype=torch.float32, device=dev)
nxt = iter(range(n_steps))


def stepper(seg, stream=None):
    latents = torch.randn(1, C, T, Hl, Wl, generator=g).to(BF16).to(dev)

    def step_fn(t_buf, d_buf):
        v = model_fn_wan_video(dit, latents=latents, timestep=t_buf, context=ctx, fuse_vae_embedding_in_latents=seg)
        K.cfg_euler_dev(v[0:1], v[1:2], latents, 5.0, d_buf)
        if seg:
            latents[:, :, 0:1].copy_(first)
    return DenoiseStepper(step_fn, ts, ds, use_graph=True, stream=stream)


steppers = {"plain": stepper(False)}
steppers["segmented"] = stepper(True, stream=steppers["plain"].stream)
for name, st in steppers.items():
    a = timed(lambda: st(next(nxt)))
    b = timed(lambda: st(next(nxt)))
    if st.graph is None:
        raise RuntimeError(f"{name}: the step was not captured")
    print(f"{name}: eager step + capture {a:.1f} ms, first replay {b:.1f} ms", flush=True)
ms = {k: [] for k in steppers}
for _ in range(args.reps):              # interleaved repeats
    for name, st in steppers.items():
        ms[name].append(timed(lambda: st(next(nxt))))
for name in steppers:
    rec["step_" + name] = summary(ms[name])
    print(f"step {name}: {rec['step_' + name]}", flush=True)
rec["segmented_over_plain"] = round(rec["step_segmented"]["median_ms"] / rec["step_plain"]["median_ms"], 4)
print(f"first-frame segment: {rec['segmented_over_plain']} x the plain step", flush=True)
print(json.dumps(rec), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
