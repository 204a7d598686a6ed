"""Cost of a temporal-sliding-window step: ms per CFG step (hipGraph replay, 14B-dim random weights as
bench.py builds them, 832x480) of
  window : 145 frames (T = 37) under sliding_window_size 19 / stride 12 -> windows (0,19) (12,31) (24,37)
  full145: the same clip in one full-attention forward
  full73 : the 73-frame default (T = 19)
all three in one process, REPS interleaved repeats after an eager step, the capture and one replay.
The arithmetic expectation for `window` is (19 + 19 + 13) / 19 = 2.68 x full73 plus the blend.

  python tests/probes/window_step.py [--reps 3] [--only window] [--out FILE]

--only window: the windowed step alone (one eager step, the capture, --reps replays): the run to put
under `rocprofv3 --kernel-trace --stats` for the blend / gather share."""
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
from vstyler.models import VaceWanModel, WanModel, init_random_
from vstyler.pipeline import DenoiseStepper, slice_windows
from vstyler.window import plan_windows

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only", default=None, choices=("window", "full145", "full73"))
ap.add_argument("--size", type=int, default=19)
ap.add_argument("--stride", type=int, default=12)
ap.add_argument("--out", default=None, help="also write the JSON record to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
M = dict(dim=5120, ffn_dim=13824, num_heads=40, num_layers=40, vace_layers=tuple(range(0, 40, 5)))
dit = WanModel(dim=M["dim"], in_dim=16, ffn_dim=M["ffn_dim"], out_dim=16, text_dim=4096, freq_dim=256, eps=1e-6,
               patch_size=(1, 2, 2), num_heads=M["num_heads"], num_layers=M["num_layers"], device=dev)
vace = VaceWanModel(vace_layers=M["vace_layers"], dim=M["dim"], num_heads=M["num_heads"], ffn_dim=M["ffn_dim"],
                    device=dev)
init_random_(dit, seed=5)
init_random_(vace, seed=6)
Hl, Wl = 480 // 8, 832 // 8
g = torch.Generator().manual_seed(1)
ctx = 0.1 * torch.randn(2, 512, 4096, generator=g)
ctx[0, 32:] = 0
ctx[1, 96:] = 0
ctx = ctx.to(torch.bfloat16).to(dev)
n_steps = 2 + args.reps
sched = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
sched.set_timesteps(n_steps, shift=5.0)
ts = sched.timesteps.to(torch.bfloat16).to(dev)
ds = torch.tensor([sched.delta(i) for i in range(n_steps)], dtype=torch.float32, device=dev)


def make(frames, window):
    T = (frames - 1) // 4 + 1
    latents = torch.randn(1, 16, T, Hl, Wl, generator=g).to(torch.bfloat16).to(dev)
    vc = torch.ones(1, 96, T, Hl, Wl)
    vc[:, :32] = torch.randn(1, 32, T, Hl, Wl, generator=g)
    vc = vc.to(torch.bfloat16).to(dev)
    kw = {}
    if window:
        plan = plan_windows(T, args.size, args.stride)
        print(f"T = {T}: windows {plan.windows}, weight {plan.weight.tolist()}", flush=True)
        kw = dict(sliding_window_size=args.size, sliding_window_stride=args.stride,
                  vace_context_windows=slice_windows(vc, plan))

    def step_fn(t_buf, d_buf):
        v = model_fn_wan_video(dit, vace=vace, latents=latents, timestep=t_buf, context=ctx, vace_context=vc, **kw)
        K.cfg_euler_dev(v[0:1], v[1:2], latents, 5.0, d_buf)
    return DenoiseStepper(step_fn, ts, ds, use_graph=True)


CONFIGS = {"window": (145, True), "full145": (145, False), "full73": (73, False)}
names = [args.only] if args.only else list(CONFIGS)
steppers = {}
for name in names:
    st = make(*CONFIGS[name])
    for i in range(2):                  # the eager step + capture, then one replay
        t0 = time.perf_counter()
        st(i)
        torch.cuda.synchronize()
        print(f"{name}: warm-up step {i}: {1000 * (time.perf_counter() - t0):.1f} ms "
              f"({'graph' if st.graph is not None and i else 'eager + capture'})", flush=True)
    if st.graph is None:
        raise RuntimeError(f"{name}: the step was not captured")
    steppers[name] = st

ms = {name: [] for name in names}
for r in range(args.reps):              # interleaved repeats
    for name in names:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steppers[name](2 + r)
        torch.cuda.synchronize()
        ms[name].append(1000 * (time.perf_counter() - t0))
rec = {"reps": args.reps, "size": args.size, "stride": args.stride}
for name in names:
    v = sorted(ms[name])
    rec[name] = {"ms": [round(x, 1) for x in ms[name]], "median_ms": round(v[len(v) // 2], 1),
                 "spread_ms": round(v[-1] - v[0], 1)}
    print(f"{name}: {rec[name]}", flush=True)
if "window" in rec and "full73" in rec:
    plan = plan_windows(37, args.size, args.stride)
    expect = sum(t_ - t for t, t_ in plan.windows) / 19
    ratio = rec["window"]["median_ms"] / rec["full73"]["median_ms"]
    rec["window_over_full73"] = round(ratio, 3)
    rec["expected_ratio"] = round(expect, 3)
    rec["excess_ms"] = round(rec["window"]["median_ms"] - expect * rec["full73"]["median_ms"], 1)
    print(f"window / full73 = {ratio:.3f} (frames arithmetic {expect:.3f}); excess {rec['excess_ms']} ms; "
          f"full73 repeat-to-repeat spread {rec['full73']['spread_ms']} ms", flush=True)
if "window" in rec and "full145" in rec:
    rec["window_over_full145"] = round(rec["window"]["median_ms"] / rec["full145"]["median_ms"], 3)
print(json.dumps(rec), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
