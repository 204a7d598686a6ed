"""Cost of two resident experts: ms per CFG step (hipGraph replay, 14B-dim random weights as bench.py
builds them, two DiT + VACE experts, 832x480x73) of
  single : expert 1's step, captured while expert 1 is the only model resident
  expert1: the same expert's step, captured after expert 2 was built (both resident)
  expert2: expert 2's step
and the cost of the switch itself: expert 2's first call (its eager step plus its capture; the Workspace,
the capture stream and the latents are the first expert's).  All in one process, host clock around a
synchronise, REPS interleaved repeats.  The expectation is single = expert1 = expert2.

Then vs_resize_nearest_u8 at 81 x 480x832 -> 720x1280 against torch's copy_ of the same output bytes.

  python tests/probes/two_expert_step.py [--reps 3] [--out FILE] [--skip-step]"""
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
from vstyler.pipeline import DenoiseStepper

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the JSON record to this file")
ap.add_argument("--skip-step", action="store_true", help="the resize kernel only")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
rec = {"reps": args.reps}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1000 * (time.perf_counter() - t0)


def summary(ms):
    v = sorted(ms)
    return {"ms": [round(x, 2) for x in ms], "median_ms": round(v[len(v) // 2], 2), "spread_ms": round(v[-1] - v[0], 2)}


def step_probe():
    M = dict(dim=5120, ffn_dim=13824, num_heads=40, num_layers=40, vace_layers=tuple(range(0, 40, 5)))

    def expert(seed):
        dit = WanModel(dim=M["dim"], in_dim=16, ffn_dim=M["ffn_dim"], out_dim=16, text_dim=4096, freq_dim=256,
                       eps=1e-6, patch_size=(1, 2, 2), num_heads=M["num_heads"], num_layers=M["num_layers"],
                       device=dev)
        vace = VaceWanModel(vace_layers=M["vace_layers"], dim=M["dim"], num_heads=M["num_heads"],
                            ffn_dim=M["ffn_dim"], device=dev)
        init_random_(dit, seed=seed)
        init_random_(vace, seed=seed + 1)
        return dit, vace

    Hl, Wl, T = 480 // 8, 832 // 8, 19
    g = torch.Generator().manual_seed(1)
    ctx = 0.1 * torch.randn(2, 512, 4096, generator=g)
    ctx[0, 32:] = 0
    ctx[1, 96:] = 0
    ctx = ctx.to(torch.bfloat16).to(dev)
    latents = torch.randn(1, 16, T, Hl, Wl, generator=g).to(torch.bfloat16).to(dev)
    vc = torch.ones(1, 96, T, Hl, Wl)
    vc[:, :32] = torch.randn(1, 32, T, Hl, Wl, generator=g)
    vc = vc.to(torch.bfloat16).to(dev)
    n_steps = 64
    sched = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sched.set_timesteps(n_steps, shift=5.0)
    ts = sched.timesteps.to(torch.bfloat16).to(dev)
    ds = torch.tensor([sched.delta(i) for i in range(n_steps)], dtype=torch.float32, device=dev)
    nxt = iter(range(n_steps))

    def stepper(dit, vace, stream=None):
        def step_fn(t_buf, d_buf):
            v = model_fn_wan_video(dit, vace=vace, latents=latents, timestep=t_buf, context=ctx, vace_context=vc)
            K.cfg_euler_dev(v[0:1], v[1:2], latents, 5.0, d_buf)
        return DenoiseStepper(step_fn, ts, ds, use_graph=True, stream=stream)

    def warm(name, st):
        first = timed(lambda: st(next(nxt)))
        replay = timed(lambda: st(next(nxt)))
        if st.graph is None:
            raise RuntimeError(f"{name}: the step was not captured")
        print(f"{name}: eager step + capture {first:.1f} ms, first replay {replay:.1f} ms", flush=True)
        return first

    base = torch.cuda.memory_allocated()
    e1 = expert(5)
    rec["resident_bytes_one_expert"] = torch.cuda.memory_allocated() - base
    single = stepper(*e1)
    rec["single_eager_plus_capture_ms"] = round(warm("single", single), 1)
    lone = [timed(lambda: single(next(nxt))) for _ in range(args.reps)]
    rec["single_alone"] = summary(lone)
    print(f"single (expert 2 not built yet): {rec['single_alone']}", flush=True)
    e2 = expert(7)
    rec["resident_bytes_two_experts"] = torch.cuda.memory_allocated() - base
    peak0 = torch.cuda.memory_allocated()
    st1 = stepper(*e1)
    warm("expert1", st1)
    st2 = stepper(*e2, stream=st1.stream)
    rec["switch_ms"] = round(warm("expert2 (the switch)", st2), 1)
    rec["switch_extra_bytes"] = torch.cuda.memory_allocated() - peak0
    steppers = {"single": single, "expert1": st1, "expert2": st2}
    ms = {k: [] for k in steppers}
    for _ in range(args.reps):              # interleaved repeats
        for name, st in steppers.items():
            ms[name].append(timed(lambda: st(next(nxt))))
    for name in steppers:
        rec[name] = summary(ms[name])
        print(f"{name}: {rec[name]}", flush=True)
    rec["switch_over_step"] = round(rec["switch_ms"] / rec["expert2"]["median_ms"], 3)
    print(f"resident: one expert {rec['resident_bytes_one_expert'] / 2**30:.2f} GiB, two "
          f"{rec['resident_bytes_two_experts'] / 2**30:.2f} GiB; the switch (eager step + capture) "
          f"{rec['switch_ms']} ms = {rec['switch_over_step']} replayed steps", flush=True)


def resize_probe():
    g = torch.Generator().manual_seed(2)
    src = torch.randint(0, 256, (81, 480, 832, 3), generator=g, dtype=torch.uint8).to(dev)
    out = torch.empty((81, 720, 1280, 3), dtype=torch.uint8, device=dev)
    other = torch.empty_like(out)
    K.resize_nearest_u8(src, 720, 1280, out=out)
    other.copy_(out)
    ms = {"resize": [], "copy": []}
    for _ in range(args.reps):
        ms["resize"].append(timed(lambda: K.resize_nearest_u8(src, 720, 1280, out=out)))
        ms["copy"].append(timed(lambda: other.copy_(out)))
    rec["resize_81x480x832_to_720x1280"] = summary(ms["resize"])
    rec["copy_same_bytes"] = summary(ms["copy"])
    rec["resize_out_bytes"] = out.numel()
    gbs = out.numel() / 1e6 / rec["resize_81x480x832_to_720x1280"]["median_ms"]
    print(f"resize: {rec['resize_81x480x832_to_720x1280']} ({gbs:.0f} GB/s written); "
          f"copy_ of the same bytes: {rec['copy_same_bytes']}", flush=True)


resize_probe()
if not args.skip_step:
    step_probe()
print(json.dumps(rec), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(rec) + "\n")
