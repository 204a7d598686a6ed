"""Temporal sliding window, host side: vstyler.window's plan (windows, bf16 masks, bf16 weight) against
a literal restatement of TemporalTiler_BCTHW (diffsynth/pipelines/wan_video_new.py:1207-1256), the
worked examples of DESIGN.md section 7, the argument validation (before any device work), and the
header / ctypes prototypes of the two kernels."""
import ctypes
import os
import re

import pytest
import torch

from window_util import build_1d_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def bits(t):
    return t.contiguous().view(torch.int16)


class LiteralTiler:
    """TemporalTiler_BCTHW.run with the model replaced by a recorder: the loop, the skip rule, the mask
    (window_util.build_1d_mask, :1211-1221) and the weight accumulation as the reference writes them
    (:1238-1253), data dtype bf16."""

    def run(self, T, sliding_window_size, sliding_window_stride):
        weight = torch.zeros((1, 1, T, 1, 1), dtype=BF16)
        windows, masks = [], []
        for t in range(0, T, sliding_window_stride):
            if t - sliding_window_stride >= 0 and t - sliding_window_stride + sliding_window_size >= T:
                continue
            t_ = min(t + sliding_window_size, T)
            m = build_1d_mask(t_ - t, t == 0, t_ == T, sliding_window_size - sliding_window_stride)
            mask = m.reshape(1, 1, -1, 1, 1).to(dtype=BF16)
            weight[:, :, t: t_, :, :] += mask
            windows.append((t, t_))
            masks.append(mask.reshape(-1))
        return windows, masks, weight.reshape(-1)


def test_plan_equals_the_literal_tiler_on_every_small_case():
    from vstyler.window import plan_windows
    n = 0
    for T in range(1, 25):
        for size in range(1, T + 3):
            for stride in range(1, size + 1):
                wins, masks, weight = LiteralTiler().run(T, size, stride)
                plan = plan_windows(T, size, stride)
                assert plan.windows == wins, (T, size, stride)
                assert len(plan.masks) == len(masks)
                for a, b in zip(plan.masks, masks):
                    assert a.dtype == BF16 and torch.equal(bits(a), bits(b)), (T, size, stride)
                assert plan.weight.dtype == BF16 and torch.equal(bits(plan.weight), bits(weight)), (T, size, stride)
                assert (plan.weight.float() > 0).all()
                # a ragged last window is longer than the ramp, so the reference's assignment never fails
                assert all(t_ - t > size - stride or (t == 0 and t_ == T) for t, t_ in wins), (T, size, stride)
                n += 1
    assert n > 2000


def test_worked_examples():
    from vstyler.window import plan_windows
    assert plan_windows(9, 5, 2).windows == [(0, 5), (2, 7), (4, 9)]
    assert plan_windows(9, 5, 3).windows == [(0, 5), (3, 8), (6, 9)]
    assert plan_windows(9, 4, 1).windows == [(0, 4), (1, 5), (2, 6), (3, 7), (4, 8), (5, 9)]
    assert plan_windows(7, 9, 3).windows == [(0, 7)]
    assert plan_windows(37, 19, 12).windows == [(0, 19), (12, 31), (24, 37)]
    p = plan_windows(9, 5, 2)
    # frame 4: three windows, and in the middle one the right ramp overwrote the left ramp's last value
    assert p.weight.tolist() == [1.0, 1.0, 1.0, 1.0, 1.1640625, 1.0, 1.0, 1.0, 1.0]
    assert p.masks[1].tolist() == [p.masks[2][0].item(), 0.5, p.masks[0][2].item(), 0.5, p.masks[0][4].item()]
    assert p.masks[0][:2].tolist() == [1.0, 1.0] and p.masks[2][-2:].tolist() == [1.0, 1.0]
    one = plan_windows(7, 9, 3)
    assert one.masks[0].tolist() == [1.0] * 7 and one.weight.tolist() == [1.0] * 7
    flat = plan_windows(8, 4, 4)            # no overlap: no ramps
    assert flat.windows == [(0, 4), (4, 8)] and all(m.tolist() == [1.0] * 4 for m in flat.masks)


@pytest.mark.parametrize("size,stride", [(5, None), (3, 5), (5, 0), (5, -1), (0, 0), (5.0, 3), (5, 3.0), ("5", 3),
                                         (True, True)])
def test_bad_window_arguments_are_value_errors_before_any_device_work(size, stride):
    """The pipeline holds no model and the tensors are CPU tensors: a device access would raise
    something other than ValueError (or touch self.dit = None)."""
    from vstyler import WanVideoPipeline, model_fn_wan_video
    from vstyler.window import check_window_args, plan_windows
    with pytest.raises(ValueError, match="sliding_window"):
        check_window_args(size, stride)
    with pytest.raises(ValueError):
        plan_windows(9, size, stride)
    lat = torch.zeros(1, 16, 9, 8, 12, dtype=BF16)
    ctx = torch.zeros(1, 512, 4096, dtype=BF16)
    with pytest.raises(ValueError, match="sliding_window"):
        model_fn_wan_video(None, latents=lat, timestep=torch.zeros(1), context=ctx, sliding_window_size=size,
                           sliding_window_stride=stride)
    pipe = WanVideoPipeline(device="cuda")
    with pytest.raises(ValueError, match="sliding_window"):
        pipe(prompt_emb=ctx, negative_prompt_emb=ctx, num_frames=33, height=64, width=96, sliding_window_size=size,
             sliding_window_stride=stride, output_type="latents")
    with pytest.raises(ValueError, match="sliding_window"):
        pipe.denoise(lat, ctx, ctx, sliding_window_size=size, sliding_window_stride=stride)
    with pytest.raises(ValueError, match="sliding_window"):
        pipe.denoise_unipc(lat, ctx, ctx, sliding_window_size=size, sliding_window_stride=stride)


def test_stride_alone_is_ignored():
    from vstyler.window import check_window_args
    assert check_window_args(None, 3) is None and check_window_args(None, None) is None
    assert check_window_args(5, 3) == (5, 3) and check_window_args(4, 4) == (4, 4)


def test_tea_cache_with_windows_is_not_implemented():
    from vstyler import WanVideoPipeline, model_fn_wan_video
    lat = torch.zeros(1, 16, 9, 8, 12, dtype=BF16)
    ctx = torch.zeros(1, 512, 4096, dtype=BF16)
    with pytest.raises(NotImplementedError, match="tea_cache"):
        model_fn_wan_video(None, latents=lat, timestep=torch.zeros(1), context=ctx, tea_cache=object(),
                           sliding_window_size=5, sliding_window_stride=3)
    pipe = WanVideoPipeline(device="cuda")
    with pytest.raises(NotImplementedError, match="tea_cache"):
        pipe.denoise(lat, ctx, ctx, tea_cache=object(), sliding_window_size=5, sliding_window_stride=3)


C_TYPES = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "long long": ctypes.c_longlong,
           "float": ctypes.c_float, "int": ctypes.c_int}


@pytest.mark.parametrize("name,args", [
    ("vs_window_blend", ["out", "mask", "value", "bc", "t", "l", "t0", "plane", "stream"]),
    ("vs_window_finish", ["value", "weight", "out", "bc", "t", "plane", "stream"])])
def test_header_declares_the_window_kernels_and_prototypes_match(name, args):
    from vstyler import _lib
    src = open(os.path.join(ROOT, "include", "vstyler.h")).read()
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", src, re.M)
    assert m, f"include/vstyler.h does not declare {name}"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert [p.rsplit(" ", 1)[1] for p in params] == args
    assert _lib.SIGNATURES[name] == [C_TYPES[p.rsplit(" ", 1)[0]] for p in params]
    assert name not in _lib._RESTYPES
