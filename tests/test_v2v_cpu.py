"""Video-to-video, host side: the vs_flow_add_noise declaration and its ctypes prototype agree, and
denoise_unipc rejects an out-of-range forward_step / skip_backward_step before any device work."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "long long": ctypes.c_longlong,
           "float": ctypes.c_float, "int": ctypes.c_int}


def test_header_declares_flow_add_noise_and_prototype_matches():
    from vstyler import _lib
    src = open(os.path.join(ROOT, "include", "vstyler.h")).read()
    m = re.search(r"^int\s+vs_flow_add_noise\s*\(([^)]*)\)\s*;", src, re.M)
    assert m, "include/vstyler.h does not declare vs_flow_add_noise"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    names = [p.rsplit(" ", 1)[1] for p in params]
    assert names == ["x0", "noise", "out", "n", "sigma", "fp32", "stream"]
    want = [C_TYPES[p.rsplit(" ", 1)[0]] for p in params]
    assert _lib.SIGNATURES["vs_flow_add_noise"] == want
    assert "vs_flow_add_noise" not in _lib._RESTYPES          # returns the int status like its neighbours


@pytest.mark.parametrize("fwd,back", [(0, 3), (7, 3), (4, 0), (4, 7), (-1, 3), (None, 3), (4, None), (2.0, 3)])
def test_denoise_unipc_rejects_out_of_range_steps_on_the_host(fwd, back):
    """Both counts index the 6-step schedule from its end, so they lie in [1, 6].  The pipeline holds
    no model and every tensor is a CPU tensor: the check comes before anything is moved to a device
    (a device access would raise something other than ValueError here, or touch self.dit = None)."""
    from vstyler import WanVideoPipeline
    pipe = WanVideoPipeline(device="cuda")
    lat = torch.zeros(1, 16, 2, 8, 12)
    ctx = torch.zeros(1, 512, 4096, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="forward_step|skip_backward_step"):
        pipe.denoise_unipc(lat, ctx, ctx, num_inference_steps=6, input_latents=lat.clone(), forward_step=fwd,
                           skip_backward_step=back)


def test_denoise_unipc_step_counts_need_input_latents():
    from vstyler import WanVideoPipeline
    pipe = WanVideoPipeline(device="cuda")
    lat = torch.zeros(1, 16, 2, 8, 12)
    ctx = torch.zeros(1, 512, 4096, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="input_latents"):
        pipe.denoise_unipc(lat, ctx, ctx, num_inference_steps=6, forward_step=4, skip_backward_step=3)
