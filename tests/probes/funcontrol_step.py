"""Cost of Wan-Fun control at 832x480x81 (latents 16 x 21 x 60 x 104: S = 32 760 tokens, n = 1 560 per latent
frame), B = 2 (CFG), random weights as bench.py builds them, the whole CFG step under hipGraph replay, REPS
interleaved repeats, host clock around a synchronise.

  reference: the 1.3B-dim Fun-Control step (dim 1536, in_dim 48, CLIP branch, ref_conv) with and without
             reference_latents: the grid grows from 21 to 22 frames, so the ratio should lie between 22/21
             (row-linear kernels) and (22/21)^2 (attention);
  camera:    the 1.3B-dim Control-Camera step (in_dim 32, control_adapter) with the adapter rows as the patch
             embedding's VS_EPI_RES residual against the plain step (expected 1.000), and the adapter's
             one-off time at the 1.3B and the 14B dim.

  python tests/probes/funcontrol_step.py [--reps 3] [--layers 30] [--out FILE]"""
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
from vstyler.models import SimpleAdapter, WanModel, init_random_
from vstyler.pipeline import DenoiseStepper, camera_token_rows, reference_token_rows

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--layers", type=int, default=30)
ap.add_argument("--out", default=None, help="also write the JSON record to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
BF16 = torch.bfloat16
D, HEADS, FFN = 1536, 12, 8960
T, Hl, Wl = 21, 60, 104
N = (Hl // 2) * (Wl // 2)
S = T * N
B, L = 2, 512
rec = {"S": S, "n": N, "B": B, "reps": args.reps, "layers": args.layers}
g = torch.Generator().manual_seed(1)


def summary(ms):
    v = sorted(ms)
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(v[len(v) // 2], 4), "spread_ms": round(v[-1] - v[0], 4)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1000 * (time.perf_counter() - t0)


def model(in_dim, **flags):
    return init_random_(WanModel(dim=D, in_dim=in_dim, ffn_dim=FFN, out_dim=16, text_dim=4096, freq_dim=256, eps=1e-6,
                                 patch_size=(1, 2, 2), num_heads=HEADS, num_layers=args.layers, has_image_input=True,
                                 device=dev, **flags), seed=5)


ctx = 0.1 * torch.randn(2, L, 4096, generator=g)
ctx[0, 32:] = 0
ctx[1, 96:] = 0
ctx = ctx.to(BF16).to(dev)
clip = torch.randn(1, 257, 1280, generator=g).to(BF16).to(dev)
n_steps = 64
sched = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
sched.set_timesteps(n_steps, shift=5.0)
ts = sched.timesteps.to(BF16).to(dev)
ds = torch.tensor([sched.delta(i) for i in range(n_steps)], dtype=torch.float32, device=dev)
nxt = iter(range(n_steps))


def stepper(dit, y, stream=None, **const):
    latents = torch.randn(1, 16, T, Hl, Wl, generator=g).to(BF16).to(dev)

    def step_fn(t_buf, d_buf):
        v = model_fn_wan_video(dit, latents=latents, timestep=t_buf, context=ctx, y=y, clip_feature=clip, **const)
        K.cfg_euler_dev(v[0:1], v[1:2], latents, 5.0, d_buf)
    return DenoiseStepper(step_fn, ts, ds, use_graph=True, stream=stream)


def compare(tag, steppers):
    for name, st in steppers.items():
        a = timed(lambda: st(next(nxt)))
        b = timed(lambda: st(next(nxt)))
        if st.graph is None:
            raise RuntimeError(f"{name}: the step was not captured")
        print(f"{tag} {name}: eager step + capture {a:.1f} ms, first replay {b:.1f} ms", flush=True)
    ms = {k: [] for k in steppers}
    for _ in range(args.reps):              # interleaved repeats
        for name, st in steppers.items():
            ms[name].append(timed(lambda: st(next(nxt))))
    for name in steppers:
        rec[f"{tag}_{name}"] = summary(ms[name])
        print(f"{tag} step {name}: {rec[f'{tag}_{name}']}", flush=True)


# ---- the reference frame
dit = model(48, has_ref_conv=True)
y = torch.randn(1, 32, T, Hl, Wl, generator=g).to(BF16).to(dev)
ref = reference_token_rows(dit, torch.randn(1, 16, 1, Hl, Wl, generator=g).to(BF16).to(dev))
st = {"plain": stepper(dit, y)}
st["reference"] = stepper(dit, y, stream=st["plain"].stream, reference_tokens=ref)
compare("ref", st)
rec["reference_over_plain"] = round(rec["ref_reference"]["median_ms"] / rec["ref_plain"]["median_ms"], 4)
print(f"reference frame: {rec['reference_over_plain']} x the plain step (22/21 = {22 / 21:.4f}, "
      f"(22/21)^2 = {(22 / 21) ** 2:.4f})", flush=True)
del st, dit, y, ref
torch.cuda.empty_cache()

# ---- camera control
dit = model(32, add_control_adapter=True)
y = torch.randn(1, 16, T, Hl, Wl, generator=g).to(BF16).to(dev)
cam_in = torch.randn(1, 24, T, 8 * Hl, 8 * Wl, generator=g).to(BF16).to(dev)
one_off = [timed(lambda: camera_token_rows(dit, cam_in, B)) for _ in range(args.reps + 1)][1:]
rec["adapter_1p3b"] = summary(one_off)
print(f"camera adapter, dim {D}, once per call: {rec['adapter_1p3b']}", flush=True)
cam = camera_token_rows(dit, cam_in, B)
st = {"plain": stepper(dit, y)}
st["camera"] = stepper(dit, y, stream=st["plain"].stream, camera_tokens=cam)
compare("cam", st)
rec["camera_over_plain"] = round(rec["cam_camera"]["median_ms"] / rec["cam_plain"]["median_ms"], 4)
print(f"camera control (VS_EPI_RES patch embedding): {rec['camera_over_plain']} x the plain step", flush=True)
del st, dit, cam
torch.cuda.empty_cache()
big = init_random_(SimpleAdapter(24, 5120, device=dev), seed=5)
one_off = [timed(lambda: big(cam_in)) for _ in range(args.reps + 1)][1:]
rec["adapter_14b"] = summary(one_off)
print(f"camera adapter, dim 5120, once per call: {rec['adapter_14b']}", flush=True)

print(json.dumps(rec), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
