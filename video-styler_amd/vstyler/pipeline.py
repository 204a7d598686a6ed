"""WanVideoPipeline with the reference call surface (diffsynth/pipelines/wan_video_new.py:32-560), running on
libvstyler kernels; model_fn_wan_video (:1260-1468) is vstyler.forward's, importable from here as before.

Differences from the reference that are performance-only (same per-sample arithmetic):
  * CFG runs as one batch-2 forward (posi, nega) instead of two batch-1 forwards; the per-batch
    head modulation (mod + t[b]) equals the reference's batch-1 broadcast (wan_video_dit.py:267);
  * sigma table on the host, Euler+CFG fused into one kernel (no per-step host sync);
  * Ulysses SP shards the VACE branch too (the reference runs VACE unsharded).
"""
import functools
import os
from dataclasses import dataclass
from typing import Optional, Union

import torch

from . import kernels as K
from .flow_match import FlowMatchScheduler
from .forward import (_UNSUPPORTED, _workspace, camera_token_rows, check_support,  # noqa: F401 (re-exported)
                      model_fn_wan_video, reference_token_rows, slice_windows)
from .models import IMG_TOKENS, WanModel, VaceWanModel
from .options import host_option
from .window import check_window_args, plan_windows

BF16 = torch.bfloat16


def fun_control_y(control_latents, y, clip_feature, in_dim, keep_clip=False):
    """WanVideoUnit_FunControl.process (wan_video_new.py:766-773) -> (y, clip_feature): y = cat([control
    latents, y_rest]) with y_dim = in_dim - 16 - 16 channels of y_rest -- the last y_dim channels of the
    image y when both y and clip_feature exist, otherwise zeros, and clip_feature then zeros [1, 257, 1280].
    keep_clip: clip_feature was given explicitly by the caller and is never replaced."""
    y_dim = in_dim - control_latents.shape[1] - 16
    if y_dim < 0:
        raise ValueError(f"control_video: a DiT with in_dim {in_dim} has no room for 16 control channels")
    if clip_feature is None or y is None:
        if not (keep_clip and clip_feature is not None):
            clip_feature = torch.zeros((1, IMG_TOKENS, 1280), dtype=control_latents.dtype, device=control_latents.device)
        y = torch.zeros((1, y_dim) + tuple(control_latents.shape[2:]), dtype=control_latents.dtype,
                        device=control_latents.device)
    else:
        y = y[:, -y_dim:]
    return torch.cat([control_latents, y.to(control_latents.device)], dim=1).contiguous(), clip_feature


def animate_i2v_mask(mask, h, w):
    """get_i2v_mask of WanVideoPostUnit_AnimateInpaint (wan_video_new.py:1118-1127) with mask_len 0 on mask
    pixel values [F, H, W] (already 1 - mask video): nearest-resized to the latent grid (:1145: row i reads row
    floor(i H / h)), the first frame four times, then groups of four -> (4, (F + 3) / 4, h, w)."""
    F_, H, W = mask.shape
    if (F_ + 3) % 4:
        raise ValueError(f"animate_mask_video: {F_} frames are not 4 k + 1")
    ri = (torch.arange(h, device=mask.device) * H) // h
    ci = (torch.arange(w, device=mask.device) * W) // w
    m = mask[:, ri][:, :, ci]
    m = torch.cat([m[0:1].expand(4, h, w), m[1:]], dim=0)
    return m.view((F_ + 3) // 4, 4, h, w).transpose(0, 1).contiguous()


def animate_inpaint_y(ref_latents, bg_latents, mask):
    """The y of WanVideoPostUnit_AnimateInpaint (wan_video_new.py:1129-1151) from its encoded parts:
    ref_latents (1, 16, 1, h, w) of input_image under a mask of ones (y_ref), then bg_latents (1, 16, T, h, w)
    of the inpaint video under animate_i2v_mask(mask) (y_reft) -> (1, 20, 1 + T, h, w) bf16."""
    _, _, T, h, w = bg_latents.shape
    dev = bg_latents.device
    y_ref = torch.cat([torch.ones((4, 1, h, w), device=dev, dtype=BF16), ref_latents[0].to(device=dev, dtype=BF16)])
    msk = animate_i2v_mask(mask.to(dev), h, w).to(BF16)
    if msk.shape[1] != T:
        raise ValueError(f"animate_mask_video covers {msk.shape[1]} latent frames, animate_inpaint_video {T}")
    y_reft = torch.cat([msk, bg_latents[0].to(BF16)])
    return torch.cat([y_ref, y_reft], dim=1).unsqueeze(0).contiguous()


def animate_face_motion_batch(motion, motion_uncond, use_cfg):
    """The face motion of a step's batch: motion [T_face, C] or [1, T_face, C]; with CFG the unconditioned
    sample's rows behind it -- motion_uncond [C], [1, C] (one vector, the motion of the reference's constant
    -1 face frame, broadcast over time), [T_face, C] or [1, T_face, C].  -> [1 or 2, T_face, C]."""
    m = motion if motion.dim() == 3 else motion[None]
    if m.dim() != 3 or m.shape[0] != 1:
        raise ValueError(f"animate_face_motion: expected [T_face, C] or [1, T_face, C], got {tuple(motion.shape)}")
    if not use_cfg:
        return m
    if motion_uncond is None:
        raise ValueError("animate_face_motion with cfg_scale != 1 needs animate_face_motion_uncond= (the motion "
                         "vector of the reference's constant -1 face frame, which its unconditioned sample sees)")
    u = motion_uncond.to(m.device)
    T, C = m.shape[1], m.shape[2]
    if u.shape[-1] != C or u.numel() not in (C, T * C):
        raise ValueError(f"animate_face_motion_uncond: expected [{C}] or [{T}, {C}], got {tuple(motion_uncond.shape)}")
    u = u.reshape(1, -1, C).expand(1, T, C)
    return torch.cat([m, u.to(m.dtype)], dim=0)


def image_mask(num_frames, h, w, has_end=False, device=None, dtype=BF16):
    """The 4 mask channels of y (wan_video_new.py:709-720) -> (4, T', h, w), T' = (num_frames + 3) / 4:
    pixel frame f is known (1) when it is the input image (f = 0) or the end image (f = num_frames - 1),
    the first frame counts four times, and latent frame t's channel c is frame 4t + c of that list."""
    known = torch.zeros(num_frames + 3, dtype=dtype, device=device)
    known[:4] = 1
    if has_end:
        known[-1] = 1
    if known.numel() % 4:
        raise ValueError(f"num_frames must be 4k + 1, got {num_frames}")
    return known.view(-1, 4).t()[:, :, None, None].expand(4, known.numel() // 4, h, w).contiguous()


def image_vae_input(image, end_image, num_frames):
    """The VAE input of the image embedder (wan_video_new.py:713-717): image (and end_image) are
    normalised (1, 3, 1, H, W) frames; the frames between / after them are zeros -> (1, 3, num_frames, H, W)."""
    B, C, _, H, W = image.shape
    gap = num_frames - (1 if end_image is None else 2)
    if gap < 0:
        raise ValueError(f"num_frames {num_frames} cannot hold the input and end images")
    parts = [image, torch.zeros((B, C, gap, H, W), dtype=image.dtype, device=image.device)]
    if end_image is not None:
        parts.append(end_image)
    return torch.cat(parts, dim=2)


@dataclass
class ModelConfig:
    """diffsynth/utils/__init__.py:158-218, offline: resolves local files only (no ModelScope)."""
    path: Union[str, list, None] = None
    model_id: str = None
    origin_file_pattern: Union[str, list, None] = None
    download_resource: str = "ModelScope"
    offload_device: Optional[Union[str, torch.device]] = None
    offload_dtype: Optional[torch.dtype] = None
    local_model_path: str = None
    skip_download: bool = False

    def download_if_necessary(self, use_usp=False):
        if isinstance(self.path, str) and any(ch in self.path for ch in "*?["):
            import glob
            files = sorted(glob.glob(self.path))
            if not files:
                raise FileNotFoundError(f"no local files match {self.path}")
            self.path = files[0] if len(files) == 1 else files
        if self.path is not None:
            return
        if self.model_id is None:
            raise ValueError('No valid model files. Please use `ModelConfig(path="xxx")` or '
                             '`ModelConfig(model_id="xxx/yyy", origin_file_pattern="zzz")`.')
        import glob
        root = os.path.join(self.local_model_path or "./models", self.model_id)
        pattern = self.origin_file_pattern or ""
        if pattern == "" or pattern.endswith("/"):
            self.path = os.path.join(root, pattern)
            if not os.path.isdir(self.path):
                raise FileNotFoundError(f"{self.path} not found (offline build: no ModelScope download)")
            return
        files = sorted(glob.glob(os.path.join(root, pattern)))
        if not files:
            raise FileNotFoundError(f"no local files match {os.path.join(root, pattern)} "
                                    "(offline build: no ModelScope download)")
        self.path = files[0] if len(files) == 1 else files


# wan_video_new.py:352-363: the files every Wan2.1 release ships identically are read from one
# model_id, so a ./models tree laid out by the reference's downloads holds them only there
REDIRECT_COMMON_FILES = {
    "models_t5_umt5-xxl-enc-bf16.pth": "Wan-AI/Wan2.1-T2V-1.3B",
    "Wan2.1_VAE.pth": "Wan-AI/Wan2.1-T2V-1.3B",
    "models_clip_open-clip-xlm-roberta-large-vit-huge-14.pth": "Wan-AI/Wan2.1-I2V-14B-480P",
}


def redirect_model_configs(model_configs):
    """Rewrites model_id in place for the common files, with the reference's notice
    (wan_video_new.py:352-363).  Configs without a model_id or file pattern are left alone."""
    for mc in model_configs:
        if mc.origin_file_pattern is None or mc.model_id is None:
            continue
        if not isinstance(mc.origin_file_pattern, str):
            continue
        target = REDIRECT_COMMON_FILES.get(mc.origin_file_pattern)
        if target is not None and mc.model_id != target:
            print(f"To avoid repeatedly downloading model files, ({mc.model_id}, {mc.origin_file_pattern}) is "
                  f"redirected to ({target}, {mc.origin_file_pattern}). You can use `redirect_common_files=False` "
                  "to disable file redirection.")
            mc.model_id = target


def sp_graph_ok(plan):
    """True when the sequence-parallel plan's collectives can be captured into the step's hipGraph:
    host options sp_graph=1 and sp_comm=native (RCCL through libvstyler's vs_sp_*) -- not
    torch.distributed's RCCL, whose process-group stream the capture does not survive on this
    image's HIP (segfault in hipStreamEndCapture, profiles/r3/sp_graph_probe_faulthandler.log), and
    not host-staged substitutes (tests).  NativeComm in side-stream mode keeps its exchange/compute
    overlap in the graph: DenoiseStepper binds its comm stream to the capture origin and forks the
    compute (usp.NativeComm).  Opt-in: only world size 1 has run on hardware
    (test_ulysses_rccl_world1_graph_capture); SP steps run eager by default."""
    if not host_option("sp_graph"):
        return False
    if plan is None:
        from .usp import get_default_group
        plan = get_default_group()
    if plan is None:
        return True
    return all(getattr(p, "capturable", True) for p in
               (plan, getattr(plan, "ulysses", None), getattr(plan, "full", None)) if p is not None)


class DenoiseStepper:
    """Runs CFG denoising steps over device-resident state.  `step_fn(t_buf, d_buf)` enqueues one
    whole step (model_fn + fused CFG/Euler) reading the bf16 timestep and the fp32 dsigma from the
    two device slots.  The first call runs eagerly (sizing every Workspace buffer); the step is then
    captured once into a hipGraph and every later call refreshes the two slots and replays it.
    The eager step and the capture run on one dedicated stream, so the split-tail workspaces that
    libvstyler keeps per (device, stream) and allocates in the eager step are the ones the captured
    launches use (a capture on a fresh stream could not allocate them and would launch unsplit).

    comms: side-stream NativeComm objects of an SP plan (usp.plan_native_comms).  With a graph they
    are bound to the stepper's stream -- the capture origin -- and the step's compute runs on a
    second stream forked from it and joined back, so the collectives overlap the compute inside
    the graph while RCCL itself only ever runs on the origin stream.  plan: the step's SP plan (None
    without SP): the capture is refused while a side-stream communicator reachable from it is not
    bound to the capture stream (usp.unbound_side_comms).

    A graph holds the weight pointers of the model it captured, so a loop over two experts runs one
    stepper per expert segment (WanVideoPipeline.denoise)."""

    def __init__(self, step_fn, timesteps_bf16, dsigmas_f32, use_graph=True, on_replay=None, comms=(), plan=None,
                 stream=None):
        self.step_fn, self.ts, self.ds = step_fn, timesteps_bf16, dsigmas_f32
        self.t_buf, self.d_buf = timesteps_bf16[0:1].clone(), dsigmas_f32[0:1].clone()
        self.use_graph, self.graph, self.on_replay = use_graph, None, on_replay
        dev = self.t_buf.device
        # stream: the dedicated stream of an earlier stepper of the same loop (one per expert segment),
        # so every segment's eager step and capture find the split-tail workspaces of the first
        if not use_graph:
            self.stream = None
        else:
            self.stream = stream if stream is not None else torch.cuda.Stream(device=dev)
        self.comms = list(comms) if use_graph else []
        self.plan = plan
        self.compute = torch.cuda.Stream(device=dev) if self.comms else None

    def _run(self):
        if self.compute is None:
            self.step_fn(self.t_buf, self.d_buf)
            return
        self.compute.wait_stream(self.stream)          # fork
        with torch.cuda.stream(self.compute):
            self.step_fn(self.t_buf, self.d_buf)
        self.stream.wait_stream(self.compute)          # join

    def __call__(self, i):
        self.t_buf.copy_(self.ts[i:i + 1])
        self.d_buf.copy_(self.ds[i:i + 1])
        if self.graph is not None:
            self.graph.replay()
            if self.on_replay is not None:
                self.on_replay()
            return
        if not self.use_graph:
            self.step_fn(self.t_buf, self.d_buf)
            return
        cur = torch.cuda.current_stream(self.t_buf.device)
        self.stream.wait_stream(cur)
        old = [c.bind_stream(self.stream) for c in self.comms]
        try:
            with torch.cuda.stream(self.stream):
                self._run()
                self.capture()
        finally:
            for c, s in zip(self.comms, old):
                c.bind_stream(s)
        cur.wait_stream(self.stream)

    def capture(self):
        g = torch.cuda.CUDAGraph()
        err = None
        stray = []
        if self.plan is not None:
            from .usp import unbound_side_comms
            stray = unbound_side_comms(self.stream, self.plan)
        if stray:                   # RCCL forked into the capture from a side stream: never capture
            err = RuntimeError(f"{len(stray)} side-stream communicator(s) not bound to the capture stream")
        else:
            try:
                with torch.cuda.graph(g, stream=self.stream):
                    self._run()
            except Exception as e:      # e.g. a collective backend that cannot be captured: stay eager
                err = e
        # the decision is collective: with several ranks replaying graphs whose collectives must
        # pair up, one rank falling back to eager steps while the others replay would deadlock or
        # mismatch, so every rank keeps its graph only if every rank captured one
        if not self._all_ranks_agree(err is None):
            import warnings
            why = repr(err) if err is not None else "another rank's capture failed"
            warnings.warn(f"hipGraph capture of the denoising step failed ({why}); running eager steps")
            self.use_graph = False
            return
        self.graph = g

    def _all_ranks_agree(self, ok):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return ok
        dev = self.t_buf.device if dist.get_backend() == "nccl" else torch.device("cpu")
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(flag.item())


class WanVideoPipeline:
    """The Ditto drop-in (wan_video_new.py:32).  DiT/VACE/Euler/CFG on libvstyler kernels."""

    def __init__(self, device="cuda", torch_dtype=BF16, tokenizer_path=None):
        self.device = device
        self.torch_dtype = torch_dtype
        self.scheduler = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
        self.text_encoder = None
        self.prompter = None
        self.image_encoder = None
        self.dit: WanModel = None
        self.dit2 = None
        self.vae = None
        self.vace: VaceWanModel = None
        self.vace2 = None
        self.motion_controller = None
        self.animate_adapter = None
        self.model_fn = model_fn_wan_video
        self.height_division_factor = 16
        self.width_division_factor = 16
        self.time_division_factor = 4
        self.time_division_remainder = 1
        self.use_unified_sequence_parallel = False
        self.sp_group = None
        self.vram_management_enabled = False

    # ---------------------------------------------------------------- loading
    @staticmethod
    def from_pretrained(torch_dtype=BF16, device="cuda", model_configs=(), tokenizer_config=None,
                        audio_processor_config=None, redirect_common_files=True, use_usp=False,
                        fp8_weights="fold"):
        """wan_video_new.py:341-413 (local files only).  fp8_weights: what becomes of a checkpoint's
        e4m3 tensors, "fold" (bf16 weights only) or "keep" (the block Linears also run the file's own
        bytes and scales on the fp8 GEMMs): loader.load_models."""
        from .loader import load_models
        if redirect_common_files:
            redirect_model_configs(model_configs)
        pipe = WanVideoPipeline(device=device, torch_dtype=torch_dtype)
        if use_usp:
            pipe.initialize_usp()
            device = pipe.device
        paths = []
        for mc in model_configs:
            mc.download_if_necessary(use_usp=use_usp)
            paths.append(mc.path)
        models = load_models(paths, device=device, fp8_weights=fp8_weights)
        pipe.dit = models.get("wan_video_dit")
        pipe.vace = models.get("wan_video_vace")
        # the second expert of a Wan2.2 A14B pair, in file order (fetch_model(..., index=2), :381-391)
        pipe.dit2 = models.get("wan_video_dit2")
        pipe.vace2 = models.get("wan_video_vace2")
        pipe.animate_adapter = models.get("wan_video_animate_adapter")
        pipe.vae = models.get("wan_video_vae")
        pipe.text_encoder = models.get("wan_video_text_encoder")
        pipe.image_encoder = models.get("wan_video_image_encoder")
        if pipe.text_encoder is not None:
            from .t5 import WanPrompter
            tok = None
            if tokenizer_config is None:
                # the reference's default (wan_video_new.py:346): ./models/Wan-AI/Wan2.1-T2V-1.3B/google/*
                tokenizer_config = ModelConfig(model_id="Wan-AI/Wan2.1-T2V-1.3B", origin_file_pattern="google/*")
                try:
                    tokenizer_config.download_if_necessary()
                    tok = tokenizer_config.path
                except FileNotFoundError:
                    tok = None   # no local tokenizer: prompts need encode_ids / prompt_emb=
            else:
                tokenizer_config.download_if_necessary()
                tok = tokenizer_config.path
            if isinstance(tok, list):
                tok = os.path.dirname(tok[0])
            pipe.prompter = WanPrompter(tokenizer_path=tok)
            pipe.prompter.fetch_models(pipe.text_encoder)
        if use_usp:
            pipe.enable_usp()
        return pipe

    def load_lora(self, module, lora_config=None, alpha=1, hotload=False, state_dict=None):
        """wan_video_new.py:80-106.  hotload=True on a quantize_fp8_ model keeps the adapter un-merged
        behind the fp8 GEMMs (layers.py:168-182), as the reference's fp8 workflows do."""
        from .lora import load_lora_state_dict, merge_lora, hotload_lora
        lora = state_dict if state_dict is not None else load_lora_state_dict(lora_config, self.device)
        if hotload:
            return hotload_lora(module, lora, alpha, fp8_layers="fuse")
        return merge_lora(module, lora, alpha)

    def enable_vram_management(self, num_persistent_param_in_dit=None, vram_limit=None, vram_buffer=0.5):
        """wan_video_new.py:124.  On MI355X (288 GB HBM) every weight stays resident, so there is no
        offload state machine; LayerNorms already run in fp32 (WanAutoCastLayerNorm semantics)."""
        self.vram_management_enabled = True

    def initialize_usp(self):
        from .usp import init_distributed
        rank = init_distributed()
        self.device = f"cuda:{rank}"

    def enable_usp(self):
        from .usp import get_default_group
        self.sp_group = get_default_group()
        self.use_unified_sequence_parallel = True

    # ---------------------------------------------------------------- helpers
    def latent_geometry(self, output_type=None):
        """(latent channels, spatial stride) of the loaded models: the VAE's when there is one, otherwise
        the DiT's out_dim -- 16 channels at stride 8 (Wan2.1 VAE), or 48 at stride 16 (the Wan2.2 VAE of
        TI2V-5B, wan_video_new.py:583).  output_type: what a __call__ is to return -- when the VAE and the
        DiT disagree the DiT's latents can be produced ("latents": the DiT's geometry) but not decoded
        (anything else: RuntimeError)."""
        dit = self.dit if self.dit is not None else self.dit2
        z = self.vae.z_dim if self.vae is not None else (dit.out_dim if dit is not None else 16)
        if output_type is not None and self.vae is not None and dit is not None and dit.out_dim != z:
            if output_type != "latents":
                raise RuntimeError(f"the loaded VAE decodes {z}-channel latents, the DiT produces {dit.out_dim}: "
                                   f"use output_type=\"latents\"")
            z = dit.out_dim
        return (48, 16) if z == 48 else (16, 8)

    def check_resize_height_width(self, height, width, num_frames=None, output_type=None):
        """utils/__init__.py:43-57; height / width round up to twice the latent stride when that is 16
        (wan_video_new.py:399-400: 32).  output_type: as latent_geometry."""
        if self.latent_geometry(output_type)[1] == 16:
            height, width = (height + 31) // 32 * 32, (width + 31) // 32 * 32
        if height % self.height_division_factor != 0:
            height = (height + self.height_division_factor - 1) // self.height_division_factor * self.height_division_factor
        if width % self.width_division_factor != 0:
            width = (width + self.width_division_factor - 1) // self.width_division_factor * self.width_division_factor
        if num_frames is None:
            return height, width
        if num_frames % self.time_division_factor != self.time_division_remainder:
            num_frames = (num_frames + self.time_division_factor - 1) // self.time_division_factor * \
                self.time_division_factor + self.time_division_remainder
        return height, width, num_frames

    def generate_noise(self, shape, seed=None, rand_device="cpu", rand_torch_dtype=torch.float32):
        """utils/__init__.py:117-122 (same CPU generator stream -> identical noise)."""
        generator = None if seed is None else torch.Generator(rand_device).manual_seed(seed)
        noise = torch.randn(shape, generator=generator, device=rand_device, dtype=rand_torch_dtype)
        return noise.to(dtype=self.torch_dtype, device=self.device)

    # ---------------------------------------------------------------- denoise
    def _expert(self, e):
        """(dit, vace) of expert 1 or 2; an expert the plan never selects is never looked at."""
        dit, vace = (self.dit, self.vace) if e == 1 else (self.dit2, self.vace2)
        if dit is None:
            raise RuntimeError(f"the schedule selects expert {e}, but pipe.dit{'' if e == 1 else '2'} is not loaded")
        return dit, vace

    def denoise(self, latents, context_posi, context_nega, vace_context=None, vace_scale=1.0, cfg_scale=5.0,
                num_inference_steps=50, sigma_shift=5.0, denoising_strength=1.0, progress_bar_cmd=None,
                use_graph=None, tea_cache=None, sliding_window_size=None, sliding_window_stride=None,
                switch_DiT_boundary=0.875, y=None, clip_feature=None, first_frame_latents=None,
                reference_latents=None, control_camera_latents_input=None, pose_latents=None,
                animate_face_motion=None, animate_face_motion_uncond=None):
        """The loop of wan_video_new.py:515-542 (cfg_merge batched), returns the final latents.

        pose_latents [1, 16, T - 1, h, w] / animate_face_motion [1, T_face, 512] (Wan2.2-Animate, with
        pipe.animate_adapter; model_fn_wan_video): computed once before the loop -- the pose rows, the face
        encoder and every fuser block's keys and values, which live in workspace buffers that the captured
        step reads and the next call overwrites.  With CFG the unconditioned sample attends the keys of
        animate_face_motion_uncond (required then).  What does not run together (NotImplementedError) is
        forward.EXCLUDES, checked before anything is computed (_forward_keywords).

        reference_latents [1, 16, (1,) h, w] / control_camera_latents_input [1, 24, T, H, W] (Wan-Fun
        control, model_fn_wan_video): neither depends on the step, so each expert's ref_conv tokens and
        camera adapter rows are computed once, before the loop, and every step -- eager or captured --
        reads them as constants, like y.

        first_frame_latents [1, C, 1, h, w] (a fuse_vae_embedding_in_latents DiT, Wan2.2-TI2V-5B): the
        clean latents of the first frame.  Written into frame 0 of the start latents (:747), every forward
        runs with fuse_vae_embedding_in_latents=True (frame 0's tokens at timestep 0) and frame 0 is set
        back to them after each scheduler step (:541-542), inside the captured step too.

        y / clip_feature: the image conditioning of an I2V DiT (model_fn_wan_video), constant over the
        steps and handed to both experts; y is cut per window once, like the vace_context.

        Step 0 runs eagerly (it also sizes the Workspace); the whole step -- model_fn (DiT + VACE,
        CFG as one batch-2 forward) + fused CFG/Euler update -- is then captured once into a hipGraph
        (torch.cuda.CUDAGraph over hipStreamBeginCapture) and replayed for every later step.  The
        graph reads the step's bf16 timestep and fp32 dsigma from two device slots refreshed before
        each replay, so one capture serves all steps.  Under Ulysses SP the RCCL collectives (async
        all-to-alls on RCCL's stream, event-ordered) are captured with the step only with host option
        sp_graph=1 (sp_graph_ok); eager with use_graph=False / host option graph=0.

        sliding_window_size / sliding_window_stride go to model_fn inside the step, so one capture
        holds all windows of a step; the vace_context is cut per window once, here.

        Two experts (dit2 set; wan_video_new.py:518-523): the steps whose fp32 timestep is below
        switch_DiT_boundary * 1000 run on dit2 / vace2 (experts.plan_experts; vace2 None: no hints,
        as the reference's models["vace"] = self.vace2).  Every segment of the plan is the loop above
        on its own: first step eager, then captured and replayed (a graph holds one expert's weight
        pointers), unless it has a single step.  The segments share the Workspace, the capture stream
        and the latents.  cfg_scale may be a (low_noise, high_noise) pair: dit takes [1], dit2 [0]; a
        segment whose scale is exactly 1.0 runs the batch-1 forward.  last_graphs: every segment's
        graph (None for an eager one); last_graph: the last segment's."""
        from .experts import expert_cfg_scales, plan_experts
        has2 = self.dit2 is not None
        scales = expert_cfg_scales(cfg_scale, has2)
        keywords, ffl = self._forward_keywords(
            "WanVideoPipeline.denoise", latents, context_posi, context_nega, vace_context, vace_scale,
            (sliding_window_size, sliding_window_stride), y, clip_feature, reference_latents,
            control_camera_latents_input, tea_cache, first_frame_latents, pose_latents, animate_face_motion,
            animate_face_motion_uncond)
        self.scheduler.set_timesteps(num_inference_steps, denoising_strength=denoising_strength, shift=sigma_shift)
        n_steps = len(self.scheduler.timesteps)
        segments = plan_experts(self.scheduler.timesteps, switch_DiT_boundary, has2)
        if use_graph is None:
            use_graph = bool(host_option("graph"))
        # TeaCache decides per step on the host (wan_video_new.py:1173-1192): eager steps
        use_graph = use_graph and tea_cache is None and \
            (not self.use_unified_sequence_parallel or sp_graph_ok(self.sp_group))
        latents = latents.to(device=self.device, dtype=BF16).contiguous().clone()
        if ffl is not None:
            latents[:, :, 0:1].copy_(ffl)                                                # :747
        ts = self.scheduler.timesteps.to(dtype=BF16).to(self.device)                     # :526
        ds = torch.tensor([self.scheduler.delta(i) for i in range(n_steps)], dtype=torch.float32,
                          device=self.device)

        def make_step(e, scale):
            use_cfg = scale != 1.0
            kw = keywords(e, use_cfg)       # the expert's constants: computed here, outside any capture

            def step(t_buf, d_buf):
                v = self.model_fn(latents=latents, timestep=t_buf, **kw)
                K.cfg_euler_dev(v[0:1], v[1:2] if use_cfg else None, latents, scale, d_buf)
                if ffl is not None:
                    latents[:, :, 0:1].copy_(ffl)                                        # :541-542
            return step

        plan = None
        if self.use_unified_sequence_parallel:
            from .usp import get_default_group, plan_native_comms
            plan = self.sp_group if self.sp_group is not None else get_default_group()
        steppers = []
        stream = None
        for first, last, e in segments:
            seg_graph = use_graph and last > first
            comms = plan_native_comms(plan) if plan is not None and seg_graph else ()
            st = DenoiseStepper(make_step(e, scales[e - 1]), ts, ds, seg_graph, comms=comms, plan=plan,
                                stream=stream)
            stream = st.stream if st.stream is not None else stream
            steppers += [st] * (last - first + 1)
        steps = range(n_steps)
        if progress_bar_cmd is not None:
            steps = progress_bar_cmd(steps)
        for i in steps:
            steppers[i](i)
        self.last_graphs = [steppers[first].graph for first, _, _ in segments]
        self.last_graph = self.last_graphs[-1]
        return latents

    def _first_frame(self, first_frame_latents, latents):
        """first_frame_latents= of denoise as a device bf16 [1, C, 1, h, w] tensor (None without)."""
        if first_frame_latents is None:
            return None
        if self.dit is None or not (self.dit.fuse_vae_embedding_in_latents and self.dit.seperated_timestep):
            raise ValueError("first_frame_latents needs a DiT with fuse_vae_embedding_in_latents and "
                             "seperated_timestep (Wan2.2-TI2V-5B)")
        want = (1, latents.shape[1], 1) + tuple(latents.shape[3:])
        if tuple(first_frame_latents.shape) != want:
            raise ValueError(f"first_frame_latents: expected {want}, got {tuple(first_frame_latents.shape)}")
        return first_frame_latents.to(device=self.device, dtype=BF16).contiguous()

    def _check_control_modules(self, reference, camera):
        """Every loaded expert has the module the call's Wan-Fun conditioning needs."""
        for d in (self.dit, self.dit2):
            if d is None:
                continue
            if reference and not getattr(d, "has_ref_conv", False):
                raise ValueError("reference_image / reference_latents needs a DiT with ref_conv (has_ref_conv); "
                                 "with two experts, both")
            if camera and getattr(d, "control_adapter", None) is None:
                raise ValueError("camera control needs a DiT with control_adapter (add_control_adapter); with two "
                                 "experts, both")

    def _forward_keywords(self, who, latents, context_posi, context_nega, vace_context, vace_scale, window, y,
                          clip_feature, reference_latents, control_camera_latents_input, tea_cache=None,
                          first_frame_latents=None, pose_latents=None, animate_face_motion=None,
                          animate_face_motion_uncond=None):
        """What a sampler (`who`) hands to self.model_fn beside latents and timestep -> (keywords, ffl).

        Once per call, here: the support matrix (forward.check_support) and the module checks, before anything is
        computed; then the window keywords (window = (size, stride); vace_context and y are cut per window once),
        the image keywords as device bf16 tensors and the first-frame flag.  keywords(e, use_cfg) adds expert e's
        dit / vace, the context of the step's batch and that expert's Wan-Fun and Animate constants; they are
        computed at the first call for (e, use_cfg) and kept.  ffl: _first_frame's tensor."""
        win = check_window_args(*window)
        plan = None if win is None else plan_windows(latents.shape[2], *win)        # the call's one plan
        windows = plan is not None and len(plan.windows) > 1
        animate = pose_latents is not None or animate_face_motion is not None
        use_vace = vace_context is not None and (self.vace is not None or
                                                 (self.dit2 is not None and self.vace2 is not None))
        check_support({"animate": animate, "first_frame": first_frame_latents is not None, "windows": windows,
                       "tea_cache": tea_cache is not None, "vace": use_vace, "reference": reference_latents is not None,
                       "camera": control_camera_latents_input is not None, "dit2": self.dit2 is not None,
                       "sp": bool(self.use_unified_sequence_parallel)}, who)
        if animate and self.animate_adapter is None:
            raise ValueError("pose_latents / animate_face_motion need pipe.animate_adapter (a Wan2.2-Animate checkpoint)")
        self._check_control_modules(reference_latents is not None, control_camera_latents_input is not None)
        ffl = self._first_frame(first_frame_latents, latents)
        common = dict(vace_context=vace_context, vace_scale=vace_scale, tea_cache=tea_cache,
                      use_unified_sequence_parallel=self.use_unified_sequence_parallel, sp_group=self.sp_group)
        if win is not None:
            common.update(sliding_window_size=win[0], sliding_window_stride=win[1])
        if windows and use_vace:
            common["vace_context_windows"] = slice_windows(vace_context.to(self.device), plan)
        if windows and y is not None:
            common["y_windows"] = slice_windows(y.to(self.device), plan)
        if y is not None:
            common["y"] = y.to(device=self.device, dtype=BF16).contiguous()
        if clip_feature is not None:
            common["clip_feature"] = clip_feature.to(device=self.device, dtype=BF16).contiguous()
        if ffl is not None:
            common["fuse_vae_embedding_in_latents"] = True
        ctx_cfg = None

        @functools.lru_cache(maxsize=None)      # an expert's constants are computed at its first step and kept
        def keywords(e, use_cfg):
            nonlocal ctx_cfg
            dit, vace = self._expert(e)
            if use_cfg and ctx_cfg is None:
                ctx_cfg = torch.cat([context_posi, context_nega], 0)
            kw = dict(common, dit=dit, vace=vace, context=ctx_cfg if use_cfg else context_posi)
            # Wan-Fun: the expert's ref_conv tokens, its camera adapter rows replicated over the step's batch
            if reference_latents is not None:
                kw["reference_tokens"] = reference_token_rows(dit, reference_latents.to(self.device))
            if control_camera_latents_input is not None:
                kw["camera_tokens"] = camera_token_rows(dit, control_camera_latents_input.to(self.device),
                                                        2 if use_cfg else 1)
            # Wan2.2-Animate: the pose rows (one set for every CFG sample), every fuser block's K / V from the
            # face motion of the step's batch
            if animate:
                ad, ws = self.animate_adapter, _workspace(self.device)
                kw["animate_adapter"] = ad
            if pose_latents is not None:
                kw["pose_tokens"] = ad.pose_rows(pose_latents.to(self.device), latents.shape[2], ws)
            if animate_face_motion is not None:
                m = animate_face_motion_batch(animate_face_motion.to(self.device), animate_face_motion_uncond, use_cfg)
                kw["animate_kv"] = ad.face_kv(ad.motion_tokens(m, ws), ws)
            return kw
        return keywords, ffl

    def _face_frames(self, face_video, input_video, motion, motion_uncond):
        """animate_face_video against the rest of the call -> uint8 [T_face, size, size, 3] host frames, cut to
        len(input_video) - 4 as WanVideoPostUnit_AnimateVideoSplit does (wan_video_new.py:1065-1080)."""
        ad = self.animate_adapter
        size = None if ad is None else ad.motion_size()
        if size is None:
            raise NotImplementedError("animate_face_video needs pipe.animate_adapter with the complete motion-encoder "
                                      "weights (motion_encoder.* of a Wan2.2-Animate checkpoint): pass the face frames' "
                                      "motion vectors as animate_face_motion= [T_face, 512] (and "
                                      "animate_face_motion_uncond= with CFG)")
        if motion is not None or motion_uncond is not None:
            raise ValueError("pass animate_face_video or its motion vectors animate_face_motion= / "
                             "animate_face_motion_uncond=, not both")
        from .vae import frames_to_u8
        frames = frames_to_u8(face_video, "cpu")
        if input_video is not None:
            frames = frames[:len(input_video) - 4]
        if frames.shape[0] < 1 or tuple(frames.shape[1:3]) != (size, size):
            raise ValueError(f"animate_face_video: face frames must be {size} x {size} (the motion encoder's size; the "
                             f"reference does not resize them either), got {tuple(frames.shape)}")
        return frames

    def encode_face_video(self, frames, use_cfg):
        """Face frames uint8 [T, size, size, 3] -> (animate_face_motion [T, 512], animate_face_motion_uncond
        [512] or None): the motion encoder on the frames and, with CFG, on one constant -1 frame -- the
        reference's negative branch sees zeros_like(face_pixel_values) - 1 and frames are independent."""
        ad = self.animate_adapter
        motion = ad.encode_motion(frames.to(self.device))
        uncond = None
        if use_cfg:
            size = frames.shape[1]
            uncond = ad.encode_motion(torch.full((3, 1, size, size), -1.0, device=self.device, dtype=BF16))[0]
        return motion, uncond

    def denoise_unipc(self, latents, context_posi, context_nega, vace_context=None, vace_scale=1.0,
                      cfg_scale=1.2, num_inference_steps=4, sigma_shift=2.0, slg_blocks=(), slg_range=(0.2, 0.7),
                      progress_bar_cmd=None, input_latents=None, forward_step=None, skip_backward_step=None,
                      sliding_window_size=None, sliding_window_stride=None, switch_DiT_boundary=0.875,
                      y=None, clip_feature=None, first_frame_latents=None, reference_latents=None,
                      control_camera_latents_input=None, pose_latents=None, animate_face_motion=None,
                      animate_face_motion_uncond=None):
        """Config 5's sampler (ditto_comfyui_workflow.json WanVideoSampler 4 / 1.2 / 2.0 / unipc with
        WanVideoSLG): FlowUniPCMultistepScheduler (vstyler.unipc) on fp32 latents, CFG as one
        batch-2 forward, skip-layer guidance on the uncond sample for step fractions in slg_range.
        CFG combine in bf16 (wan_video_new.py:535 semantics), model input bf16 each step.

        input_latents: the enhancer's re-noise / partial-denoise pass (denoising_enhancing/wan/
        text2video.py:347-375): `latents` is then the noise, the loop starts from
        add_noise(input_latents, noise, timesteps[-forward_step]) and runs timesteps[-skip_backward_step:]
        (both counted from the schedule's end, in [1, n]); a step's SLG fraction stays its index in the
        full schedule over n.

        sliding_window_size / sliding_window_stride: as in denoise.

        Two experts (dit2 set): experts.plan_experts over the executed timesteps[first:] (the
        scheduler's int64 values against switch_DiT_boundary * 1000), cfg_scale a number or a
        (low_noise, high_noise) pair as in denoise.  An expert no executed step selects is never
        touched: the Wan2.2 enhancer pass (40 steps, shift 12, forward_step = skip_backward_step = 5)
        has every timestep below 875 and runs with pipe.dit = None."""
        if pose_latents is not None or animate_face_motion is not None:
            raise NotImplementedError("the animate adapter (pose_latents / animate_face_motion) with the UniPC sampler "
                                      "is not supported: use denoise (Euler)")
        from .experts import expert_cfg_scales, plan_experts
        if first_frame_latents is not None:
            raise ValueError("first_frame_latents is not supported by the UniPC sampler (use denoise)")
        has2 = self.dit2 is not None
        scales = expert_cfg_scales(cfg_scale, has2)
        # (y / clip_feature: as in denoise; the Wan-Fun constants are computed at each expert's first step)
        keywords, _ = self._forward_keywords(
            "WanVideoPipeline.denoise_unipc", latents, context_posi, context_nega, vace_context, vace_scale,
            (sliding_window_size, sliding_window_stride), y, clip_feature, reference_latents,
            control_camera_latents_input)
        from .unipc import FlowUniPCMultistepScheduler, cast
        sched = FlowUniPCMultistepScheduler(shift=1.0)
        sched.set_timesteps(num_inference_steps, shift=sigma_shift)
        n = len(sched.timesteps)
        first = 0
        if input_latents is None:
            if forward_step is not None or skip_backward_step is not None:
                raise ValueError("forward_step / skip_backward_step apply to input_latents=")
        else:
            for name, val in (("forward_step", forward_step), ("skip_backward_step", skip_backward_step)):
                if not isinstance(val, int) or isinstance(val, bool) or not 1 <= val <= n:
                    raise ValueError(f"{name} must be an integer in [1, {n}], got {val!r}")
            first = n - skip_backward_step
        expert_of = {}
        for lo, hi, e in plan_experts(sched.timesteps[first:], switch_DiT_boundary, has2):
            for i in range(first + lo, first + hi + 1):
                expert_of[i] = e
        lat32 = latents.to(device=self.device, dtype=torch.float32).contiguous().clone()
        if input_latents is not None:
            x0 = input_latents.to(device=self.device, dtype=torch.float32).contiguous()
            lat32 = sched.add_noise(x0, lat32, sched.timesteps[n - forward_step])
        lat16 = torch.empty(lat32.shape, dtype=BF16, device=self.device)
        v16 = torch.empty(lat32.shape, dtype=BF16, device=self.device)
        v32 = torch.empty_like(lat32)
        steps = range(first, n)
        if progress_bar_cmd is not None:
            steps = progress_bar_cmd(steps)
        for i in steps:
            t = sched.timesteps[i]
            cast(lat32, lat16)
            frac = i / n
            slg = tuple(slg_blocks) if slg_range[0] <= frac <= slg_range[1] else ()
            scale = scales[expert_of[i] - 1]
            use_cfg = scale != 1.0
            v = self.model_fn(latents=lat16, timestep=t.reshape(1).to(dtype=BF16, device=self.device),
                              slg_blocks=slg, **keywords(expert_of[i], use_cfg))
            v16.zero_()
            K.cfg_euler(v[0:1], v[1:2] if use_cfg else None, v16, scale, 1.0)   # v16 = cfg combine
            cast(v16, v32)
            lat32 = sched.step(v32, t, lat32)[0]
        return cast(lat32, torch.empty(lat32.shape, dtype=BF16, device=self.device))

    @torch.no_grad()
    def __call__(self, prompt=None, negative_prompt="", input_image=None, end_image=None, input_video=None,
                 denoising_strength=1.0, vace_video=None, vace_video_mask=None, vace_reference_image=None,
                 vace_scale=1.0, seed=None, rand_device="cpu", height=480, width=832, num_frames=81,
                 cfg_scale=5.0, cfg_merge=False, switch_DiT_boundary=0.875, num_inference_steps=50,
                 sigma_shift=5.0, motion_bucket_id=None, tiled=True, tile_size=(30, 52), tile_stride=(15, 26),
                 sliding_window_size=None, sliding_window_stride=None, tea_cache_l1_thresh=None,
                 tea_cache_model_id="", progress_bar_cmd=None, control_video=None, reference_image=None,
                 camera_control_direction=None, camera_control_speed=1 / 54,
                 camera_control_origin=(0, 0.532139961, 0.946026558, 0.5, 0.5, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0),
                 # extensions of this build (the DiT path without T5/VAE):
                 prompt_emb=None, negative_prompt_emb=None, vace_context=None, output_type="video",
                 input_latents=None, clip_feature=None, first_frame_latents=None, control_latents=None,
                 reference_latents=None, control_camera_latents_input=None, animate_pose_video=None,
                 animate_face_video=None, animate_inpaint_video=None, animate_mask_video=None, pose_latents=None,
                 animate_face_motion=None, animate_face_motion_uncond=None, **kwargs):
        """Wan2.2-Animate (WanVideoPostUnit_AnimatePoseLatents / AnimateFacePixelValues / AnimateInpaint,
        wan_video_new.py:1083-1151) with pipe.animate_adapter and input_image.  animate_pose_video (num_frames - 4
        frames; or its latents pose_latents [1, 16, T' - 1, h, w]) is VAE-encoded and patch-embedded onto the
        latent frames 1..; animate_face_motion [T_face, 512] are the face frames' motion vectors (the reference's
        motion encoder output; T_face = num_frames - 4) and animate_face_motion_uncond the vector of its constant
        -1 face frame, required with CFG.  animate_face_video (T_face PIL images or uint8 [size, size, 3] frames at
        the motion encoder's size, 512 for the released checkpoint; never resized) is encoded by the adapter's
        motion encoder (vstyler.motion, adapter.encode_motion) into those vectors, the constant -1 frame with it
        when CFG runs; it excludes animate_face_motion=, and is NotImplementedError without the complete
        motion_encoder.* weights.  animate_inpaint_video + animate_mask_video (num_frames - 4 frames each) replace y by the
        inpaint form (animate_inpaint_y).  With both a pose and a face motion the first latent frame is dropped
        before decoding (:545-550), so the video has num_frames - 4 frames.

        Wan-Fun control (WanVideoUnit_FunControl / FunReference / FunCameraControl, wan_video_new.py:752-845,
        in the reference's unit order).  control_video (or its precomputed control_latents [1, 16, T', h, w]):
        VAE-encoded and put in front of y, whose other in_dim - 32 channels are the last ones of the image y
        when input_image gave both y and CLIP features, else zeros -- clip_feature then defaults to zeros
        [1, 257, 1280].  reference_image (or reference_latents [1, 16, 1, h, w]) on a has_ref_conv DiT: encoded
        untiled, its ref_conv tokens lead every forward's sequence; with pipe.image_encoder loaded the CLIP
        features come from it.  camera_control_direction (with input_image; or a precomputed
        control_camera_latents_input [1, 24, T', H, W]) on a DiT with control_adapter: the trajectory's Pluecker
        rays feed the adapter once per call, and y becomes the first frame's latents (in_dim 32) or the
        mask + latents form (in_dim 36).  A precomputed tensor wins over its image form; an explicit
        clip_feature= is never replaced.

        first_frame_latents [1, C, 1, h, w]: the clean first-frame latents of a
        fuse_vae_embedding_in_latents DiT (Wan2.2-TI2V-5B image-to-video; denoise).  input_image= on such a
        DiT (WanVideoUnit_ImageEmbedderFused, wan_video_new.py:731-748) is resized, encoded by the 48-channel
        Wan2.2 VAE (WanVideoVAE38 as pipe.vae) and passed on as first_frame_latents; an explicit
        first_frame_latents= wins, and without that VAE the call raises NotImplementedError.  input_video /
        input_latents and output_type="video" go through the same VAE at its geometry (48 channels, stride 16).

        wan_video_new.py:416-560 for the Ditto path (T2V/VACE/video-to-video) and image-to-video (no
        audio/camera inputs).  input_image (and end_image) on a DiT with in_dim > 16 become y
        (encode_input_image) for both experts; a DiT that also takes CLIP features (has_image_input with
        require_clip_embedding: the Wan2.1 I2V / FLF2V / Fun-InP checkpoints) gets them from
        pipe.image_encoder (encode_clip_image; loaded by from_pretrained from the CLIP checkpoint) or
        precomputed as clip_feature= [1, 257 or 514, 1280], which wins.  With dit2 loaded the steps below switch_DiT_boundary run on dit2 / vace2 and cfg_scale
        may be a (low_noise, high_noise) pair (denoise).  input_video (or its precomputed latents input_latents (1, 16, T', h, w)) with
        denoising_strength < 1 starts the loop from the video's latents re-noised to the first sigma
        of the shortened schedule (WanVideoUnit_InputVideoEmbedder, :591-614)."""
        if motion_bucket_id is not None:
            raise NotImplementedError("motion_bucket_id is outside the Ditto hot path of this build")
        face_frames = None
        if animate_face_video is not None:                  # WanVideoPostUnit_AnimateFacePixelValues (:1099-1108)
            face_frames = self._face_frames(animate_face_video, input_video, animate_face_motion,
                                            animate_face_motion_uncond)   # (encoded below, after the checks)
        has_pose = animate_pose_video is not None or pose_latents is not None
        has_face = animate_face_motion is not None or face_frames is not None
        has_animate = has_pose or has_face or animate_inpaint_video is not None or \
            animate_mask_video is not None
        if has_animate:
            if self.animate_adapter is None:
                raise ValueError("the animate_* arguments need pipe.animate_adapter (a Wan2.2-Animate checkpoint)")
            if input_image is None:
                raise ValueError("the animate_* arguments need input_image (the character's reference image)")
            if (animate_inpaint_video is None) != (animate_mask_video is None):
                raise ValueError("animate_inpaint_video and animate_mask_video go together")
        fused = self.dit is not None and self.dit.fuse_vae_embedding_in_latents
        fused_image = None                                  # WanVideoUnit_ImageEmbedderFused's image (below)
        if input_image is not None and fused:
            if first_frame_latents is None:
                if self.vae is None or self.vae.z_dim != 48:
                    raise NotImplementedError("input_image on a fuse_vae_embedding_in_latents DiT (Wan2.2-TI2V-5B) "
                                              "needs the 48-channel Wan2.2 VAE (WanVideoVAE38) loaded as pipe.vae: "
                                              "load it, or pass the encoded first frame as first_frame_latents=")
                fused_image = input_image
            input_image = None                              # no y / CLIP branch on such a DiT
        if first_frame_latents is not None and not fused:
            raise ValueError("first_frame_latents needs a DiT with fuse_vae_embedding_in_latents (Wan2.2-TI2V-5B)")
        has_control = control_video is not None or control_latents is not None
        has_reference = reference_image is not None or reference_latents is not None
        has_camera = camera_control_direction is not None or control_camera_latents_input is not None
        self._check_control_args(has_control, has_reference, has_camera, input_image)
        self._check_image_args(input_image, end_image, clip_feature, has_control, reference_image is not None,
                               has_camera)
        if input_video is not None and input_latents is not None:
            raise ValueError("pass input_video or its precomputed input_latents, not both")
        check_window_args(sliding_window_size, sliding_window_stride)
        from .experts import expert_cfg_scales
        scales = expert_cfg_scales(cfg_scale, self.dit2 is not None)
        # (denoise checks the whole call; this pair here, before anything is encoded)
        check_support({"tea_cache": tea_cache_l1_thresh is not None, "dit2": self.dit2 is not None}, "WanVideoPipeline")
        height, width, num_frames = self.check_resize_height_width(height, width, num_frames, output_type)
        T = (num_frames - 1) // 4 + 1
        zc, zs = self.latent_geometry(output_type)
        if fused_image is not None:                         # wan_video_new.py:741-748
            first_frame_latents = self.encode_first_frame(fused_image, height, width, tiled, tile_size, tile_stride)
        # WanVideoUnit_NoiseInitializer (wan_video_new.py:578-587): f reference images add f latent
        # frames, and the noise is rolled so the last f frames come first
        nref = 0
        if vace_reference_image is not None:
            nref = len(vace_reference_image) if isinstance(vace_reference_image, (list, tuple)) else 1
        if input_video is not None or input_latents is not None:
            input_latents = self.encode_input_video(input_video, input_latents, height, width, num_frames, tiled,
                                                    tile_size, tile_stride, vace_reference_image)
        noise = self.generate_noise((1, zc, T + nref, height // zs, width // zs), seed=seed, rand_device=rand_device)
        if nref:
            noise = torch.cat((noise[:, :, -nref:], noise[:, :, :-nref]), dim=2)
        start = noise
        if input_latents is not None:                       # :484, :613: re-noise to the schedule's first sigma
            self.scheduler.set_timesteps(num_inference_steps, denoising_strength=denoising_strength, shift=sigma_shift)
            start = self.scheduler.add_noise(input_latents, noise.contiguous(), self.scheduler.timesteps[0])
        if prompt_emb is None:
            prompt_emb = self.encode_prompt(prompt)
        if negative_prompt_emb is None and any(c != 1.0 for c in scales):
            negative_prompt_emb = self.encode_prompt(negative_prompt)
        if vace_context is None and (vace_video is not None or vace_video_mask is not None or nref):
            vace_context = self.encode_vace(vace_video, vace_video_mask, height, width, num_frames, tiled,
                                            tile_size, tile_stride, vace_reference_image)
        y = None
        if input_image is not None and animate_inpaint_video is not None:     # WanVideoPostUnit_AnimateInpaint
            y = self.encode_animate_inpaint(input_image, animate_inpaint_video, animate_mask_video, height, width,
                                            num_frames, tiled, tile_size, tile_stride)
        elif input_image is not None:
            y = self.encode_input_image(input_image, end_image, num_frames, height, width, tiled, tile_size, tile_stride)
        if animate_pose_video is not None and pose_latents is None:           # WanVideoPostUnit_AnimatePoseLatents
            pose_latents = self.encode_animate_video(animate_pose_video, "animate_pose_video", height, width,
                                                     num_frames, tiled, tile_size, tile_stride)
        if face_frames is not None:                         # the motion encoder, once per call
            animate_face_motion, animate_face_motion_uncond = self.encode_face_video(
                face_frames, any(c != 1.0 for c in scales))
        # WanVideoUnit_ImageEmbedderCLIP (wan_video_new.py:682-693); an explicit clip_feature= wins
        explicit_clip = clip_feature is not None
        if clip_feature is None and input_image is not None and self.image_encoder is not None and \
                self.dit is not None and self.dit.require_clip_embedding:
            clip_feature = self.encode_clip_image(input_image, end_image, height, width)
        if has_control:                                    # WanVideoUnit_FunControl (:759-773)
            if control_latents is None:
                control_latents = self.encode_control_video(control_video, height, width, num_frames, tiled, tile_size,
                                                            tile_stride)
            y, clip_feature = fun_control_y(control_latents.to(self.device), y, clip_feature, self._main_dit().in_dim,
                                            keep_clip=explicit_clip)
        if has_reference:                                  # WanVideoUnit_FunReference (:784-795)
            if reference_latents is None:
                reference_latents = self.encode_reference_image(reference_image, height, width)
            if reference_image is not None and self.image_encoder is not None and not explicit_clip:
                clip_feature = self.image_encoder.encode_image(
                    [self._image_frame(reference_image, "reference_image", height, width)[:, :, 0]]).to(self.torch_dtype)
        if has_camera:                                     # WanVideoUnit_FunCameraControl (:806-845)
            if control_camera_latents_input is None:
                from .camera import control_camera_latents_input as camera_input
                control_camera_latents_input = camera_input(camera_control_direction, num_frames, height, width,
                                                            camera_control_speed, camera_control_origin, self.device)
            y = self.encode_camera_y(input_image, num_frames, height, width, tiled, tile_size, tile_stride, y)
        tea_cache = None
        if tea_cache_l1_thresh is not None:                # WanVideoUnit_TeaCache (:936-947)
            from .teacache import TeaCache
            tea_cache = TeaCache(num_inference_steps, rel_l1_thresh=tea_cache_l1_thresh, model_id=tea_cache_model_id)
        latents = self.denoise(start, prompt_emb.to(self.device), None if negative_prompt_emb is None else
                               negative_prompt_emb.to(self.device),
                               None if vace_context is None else vace_context.to(self.device), vace_scale,
                               cfg_scale, num_inference_steps, sigma_shift, denoising_strength, progress_bar_cmd,
                               tea_cache=tea_cache, sliding_window_size=sliding_window_size,
                               sliding_window_stride=sliding_window_stride, switch_DiT_boundary=switch_DiT_boundary,
                               y=y, clip_feature=clip_feature, first_frame_latents=first_frame_latents,
                               reference_latents=reference_latents,
                               control_camera_latents_input=control_camera_latents_input, pose_latents=pose_latents,
                               animate_face_motion=animate_face_motion,
                               animate_face_motion_uncond=animate_face_motion_uncond)
        self.last_tea_cache = tea_cache
        if nref:                                            # :545-550
            latents = latents[:, :, nref:].contiguous()
        elif has_pose and has_face:                         # :545-550: the reference image's frame
            latents = latents[:, :, 1:].contiguous()
        if output_type == "latents":
            return latents
        if self.vae is None:
            raise RuntimeError("VAE decode requires a loaded VAE (or use output_type='latents')")
        video = self.vae.decode(latents, device=self.device, tiled=tiled, tile_size=tile_size, tile_stride=tile_stride)
        return self.vae_output_to_video(video, output_type)

    @torch.no_grad()
    def enhance(self, video, prompt=None, negative_prompt="", height=720, width=1280, num_inference_steps=40,
                sigma_shift=12.0, cfg_scale=(3.0, 4.0), switch_DiT_boundary=0.875, forward_step=5,
                skip_backward_step=5, seed=None, tiled=True, tile_size=(30, 52), tile_stride=(15, 26),
                prompt_emb=None, negative_prompt_emb=None, output_type="video", first_frame_latents=None):
        """The reference's "Denoising Enhancing" mode (denoising_enhancing/video_enhancing_batch.py:43-83,
        395-419 around wan/text2video.py:297-401 with wan/configs/wan_t2v_A14B.py): frames in, frames
        out.  The video is resized to height x width (nearest neighbour, vs_resize_nearest_u8, when it is
        not that size already), VAE-encoded, re-noised at timesteps[-forward_step] of the UniPC schedule
        and denoised over timesteps[-skip_backward_step:] with the two Wan2.2 A14B experts (dit: high
        noise, dit2: low noise; per-expert guidance cfg_scale = (low_noise, high_noise)), then decoded.
        With the defaults every executed timestep is below the boundary, so only dit2 runs (pipe.dit may
        be None).  The frame count must be 4k + 1 (the reference does not round it).

        Deviations from the reference's enhancer:
          * the noise comes from generate_noise (this build's CPU generator); the reference seeds a
            device generator;
          * the negative prompt defaults to "" (the reference's config carries a fixed string);
          * frames are normalised by this build's preprocess_video (the DiffSynth pipeline's bf16
            rounding points), not by the enhancer's fp32 read_video;
          * the DiT forward keeps this build's DiffSynth rounding points; parity with the official
            Wan2.2 module (fp32 residual stream, fp32 modulation) is unpinned;
          * the DPM++ solver is not built (UniPC only).

        output_type: "video" (PIL images), "u8" ((T, H, W, 3) uint8 device tensor) or "latents"."""
        from .experts import expert_cfg_scales
        from .vae import frames_to_u8, preprocess_video
        if first_frame_latents is not None:
            raise ValueError("first_frame_latents is not supported by enhance (the UniPC sampler)")
        frames = frames_to_u8(video, self.device)
        if frames.shape[0] % 4 != 1:
            raise ValueError(f"enhance: the video must have 4k + 1 frames, got {frames.shape[0]}")
        if height % 8 or width % 8:
            raise ValueError(f"enhance: height and width must be multiples of 8, got {height}x{width}")
        scales = expert_cfg_scales(cfg_scale, self.dit2 is not None)
        if self.vae is None:
            raise RuntimeError("enhance requires a loaded Wan2.1 VAE")
        if tuple(frames.shape[1:3]) != (height, width):
            frames = K.resize_nearest_u8(frames, height, width)
        x0 = self.vae.encode(preprocess_video(frames), self.device, tiled=tiled, tile_size=tile_size,
                             tile_stride=tile_stride)
        noise = self.generate_noise(tuple(x0.shape), seed=seed)
        if prompt_emb is None:
            prompt_emb = self.encode_prompt(prompt)
        if negative_prompt_emb is None and any(c != 1.0 for c in scales):
            negative_prompt_emb = self.encode_prompt(negative_prompt)
        latents = self.denoise_unipc(noise, prompt_emb.to(self.device), None if negative_prompt_emb is None else
                                     negative_prompt_emb.to(self.device), cfg_scale=cfg_scale,
                                     num_inference_steps=num_inference_steps, sigma_shift=sigma_shift,
                                     input_latents=x0, forward_step=forward_step,
                                     skip_backward_step=skip_backward_step, switch_DiT_boundary=switch_DiT_boundary)
        if output_type == "latents":
            return latents
        out = self.vae.decode(latents, device=self.device, tiled=tiled, tile_size=tile_size, tile_stride=tile_stride)
        return self.vae_output_to_video(out, output_type)

    def encode_prompt(self, prompt):
        if self.text_encoder is None or self.prompter is None:
            raise NotImplementedError("T5 text encoder not loaded: pass prompt_emb=/negative_prompt_emb=")
        return self.prompter.encode_prompt(prompt, device=self.device)

    def _main_dit(self):
        return self.dit if self.dit is not None else self.dit2

    def _check_control_args(self, control, reference, camera, input_image):
        """The Wan-Fun arguments of __call__ against the loaded DiTs, before anything is encoded."""
        if not (control or reference or camera):
            return
        dits = [d for d in (self.dit, self.dit2) if d is not None]
        if any(d.fuse_vae_embedding_in_latents for d in dits):
            raise NotImplementedError("control_video / reference_image / camera control on a "
                                      "fuse_vae_embedding_in_latents DiT (Wan2.2-TI2V-5B)")
        if camera and input_image is None:
            raise ValueError("camera_control_direction needs input_image (the first frame)")
        for d in dits:
            if control and (d.in_dim < 32 or not d.require_vae_embedding):
                raise ValueError(f"control_video needs a Fun-Control DiT whose y holds the 16 control channels "
                                 f"(in_dim >= 32); the loaded DiT has in_dim {d.in_dim}")
            if camera and d.in_dim not in (32, 36):
                raise ValueError(f"camera control gives y 16 or 4 + 16 channels (in_dim 32 or 36); the loaded DiT has "
                                 f"in_dim {d.in_dim}")
        self._check_control_modules(reference, camera)

    def _check_image_args(self, input_image, end_image, clip_feature, control=False, reference=False, camera=False):
        """The image arguments of __call__ against the loaded DiTs, before anything is encoded.  control /
        reference / camera: the call carries that Wan-Fun conditioning (control_video and camera control
        assemble y themselves; control_video defaults clip_feature to zeros, a reference image gives its
        own when an image encoder is loaded)."""
        dits = [d for d in (self.dit, self.dit2) if d is not None]
        if end_image is not None and input_image is None:
            raise ValueError("end_image needs input_image")
        if input_image is not None:
            for d in dits:
                if d.in_dim <= 16 or not d.require_vae_embedding:
                    raise ValueError(f"input_image needs an image-to-video DiT (in_dim > 16); the loaded DiT has "
                                     f"in_dim {d.in_dim}")
                if d.in_dim != 36 and not (control or camera):
                    raise NotImplementedError(f"input_image gives the 4 + 16 channels of an in_dim 36 DiT; in_dim "
                                              f"{d.in_dim} (Fun-Control) also needs control latents")
        for d in dits:
            if control:
                continue                        # FunControl's zero clip_feature when nothing else gave one
            if reference and self.image_encoder is not None:
                continue
            if d.has_image_input and d.require_clip_embedding and clip_feature is None and \
                    (input_image is not None or d.in_dim > 16) and \
                    (self.image_encoder is None or input_image is None):
                raise ValueError("this DiT attends to CLIP image features: pass clip_feature= ([1, 257 or 514, 1280], "
                                 "the CLIP ViT-H features of the input image); this build has no image_encoder")

    def _image_frame(self, img, name, height, width):
        """One image of __call__ as the (1, 3, 1, H, W) bf16 frame in [-1, 1] of preprocess_video: a PIL
        image is resized to (width, height) with PIL's default resample, as the reference does; a uint8
        (H, W, 3) tensor / array must already be height x width."""
        from .vae import frames_to_u8, preprocess_video
        if hasattr(img, "resize") and hasattr(img, "convert"):
            img = img.resize((width, height))
        elif isinstance(img, torch.Tensor) and img.dim() == 3:
            img = img[None]
        u8 = frames_to_u8(img if isinstance(img, torch.Tensor) else [img], self.device)
        if tuple(u8.shape) != (1, height, width, 3):
            raise ValueError(f"{name} must be one {height}x{width} RGB image, got {tuple(u8.shape)}")
        return preprocess_video(u8)

    def encode_first_frame(self, input_image, height, width, tiled=True, tile_size=(30, 52), tile_stride=(15, 26)):
        """WanVideoUnit_ImageEmbedderFused (wan_video_new.py:741-748) -> first_frame_latents (1, 48, 1, h, w)
        bf16: the image as _image_frame makes it, encoded as a one-frame video by the Wan2.2 VAE."""
        image = self._image_frame(input_image, "input_image", height, width)
        z = self.vae.encode([image[0].to(self.torch_dtype)], self.device, tiled=tiled, tile_size=tile_size,
                            tile_stride=tile_stride)
        return z.to(self.torch_dtype)

    def encode_clip_image(self, input_image, end_image, height, width):
        """WanVideoUnit_ImageEmbedderCLIP (wan_video_new.py:675-693) -> clip_feature (1, 257, 1280) bf16:
        image_encoder.encode_image of the frame encode_input_image builds; end_image's features follow
        along dim 1 (514 rows) only when dit.has_image_pos_emb."""
        if self.image_encoder is None:
            raise RuntimeError("CLIP features need a loaded image_encoder (or pass clip_feature=)")
        feat = self.image_encoder.encode_image([self._image_frame(input_image, "input_image", height, width)[:, :, 0]])
        if end_image is not None and self.dit is not None and self.dit.has_image_pos_emb:
            end = self.image_encoder.encode_image([self._image_frame(end_image, "end_image", height, width)[:, :, 0]])
            feat = torch.cat([feat, end], dim=1)
        return feat.to(self.torch_dtype)

    def encode_input_image(self, input_image, end_image, num_frames, height, width, tiled=True, tile_size=(30, 52),
                           tile_stride=(15, 26)):
        """WanVideoUnit_ImageEmbedderVAE (wan_video_new.py:704-727) -> y (1, 20, T', h, w) bf16: the 4
        mask channels (image_mask) over the 16 VAE latents of [image, zeros ... (, end_image)].  A PIL
        image is resized to (width, height) with PIL's default resample, as the reference does; a uint8
        (H, W, 3) tensor / array must already be height x width."""
        if self.vae is None:
            raise RuntimeError("input_image encoding requires a loaded Wan2.1 VAE")
        image = self._image_frame(input_image, "input_image", height, width)
        end = None if end_image is None else self._image_frame(end_image, "end_image", height, width)
        vae_input = image_vae_input(image, end, num_frames)
        lat = self.vae.encode(vae_input.to(self.torch_dtype), self.device, tiled=tiled, tile_size=tile_size,
                              tile_stride=tile_stride)
        msk = image_mask(num_frames, height // 8, width // 8, end is not None, device=lat.device, dtype=lat.dtype)
        return torch.cat([msk[None], lat.to(self.torch_dtype)], dim=1).contiguous()

    def encode_control_video(self, control_video, height, width, num_frames, tiled=True, tile_size=(30, 52),
                             tile_stride=(15, 26)):
        """WanVideoUnit_FunControl's control_latents (wan_video_new.py:763-765) -> (1, 16, T', h, w) bf16.  As
        for input_video, the frames must already match the call."""
        from .vae import frames_to_u8, preprocess_video
        if self.vae is None:
            raise RuntimeError("control_video encoding requires a loaded Wan2.1 VAE (or pass control_latents=)")
        frames = frames_to_u8(control_video, self.device)
        if tuple(frames.shape) != (num_frames, height, width, 3):
            raise ValueError(f"control_video must be {num_frames} frames of {height}x{width}, got {tuple(frames.shape)}")
        return self.vae.encode(preprocess_video(frames), self.device, tiled=tiled, tile_size=tile_size,
                               tile_stride=tile_stride).to(self.torch_dtype)

    def encode_animate_video(self, video, name, height, width, num_frames, tiled=True, tile_size=(30, 52),
                             tile_stride=(15, 26)):
        """A driving video of Wan2.2-Animate (pose / inpaint: num_frames - 4 frames, one latent frame fewer than
        the latents) -> (1, 16, T' - 1, h, w) bf16 (wan_video_new.py:1094-1095, :1134-1135)."""
        from .vae import frames_to_u8, preprocess_video
        if self.vae is None:
            raise RuntimeError(f"{name} encoding requires a loaded Wan2.1 VAE")
        frames = frames_to_u8(video, self.device)
        if tuple(frames.shape) != (num_frames - 4, height, width, 3):
            raise ValueError(f"{name} must be {num_frames - 4} frames (num_frames - 4) of {height}x{width}, got "
                             f"{tuple(frames.shape)}")
        return self.vae.encode(preprocess_video(frames), self.device, tiled=tiled, tile_size=tile_size,
                               tile_stride=tile_stride).to(self.torch_dtype)

    def encode_animate_inpaint(self, input_image, inpaint_video, mask_video, height, width, num_frames, tiled=True,
                               tile_size=(30, 52), tile_stride=(15, 26)):
        """WanVideoPostUnit_AnimateInpaint (wan_video_new.py:1129-1151) -> y (1, 20, T', h, w) bf16: the reference
        image's latents under a mask of ones, then the inpaint video's under 1 - mask video (channel 0 of its
        frames scaled to [0, 1]), nearest-resized to the latent grid."""
        from .vae import frames_to_u8
        bg = self.encode_animate_video(inpaint_video, "animate_inpaint_video", height, width, num_frames, tiled,
                                       tile_size, tile_stride)
        frame = self._image_frame(input_image, "input_image", height, width)
        ref = self.vae.encode(frame.to(self.torch_dtype), self.device, tiled=tiled, tile_size=tile_size,
                              tile_stride=tile_stride).to(self.torch_dtype)
        m8 = frames_to_u8(mask_video, self.device)
        if tuple(m8.shape) != (num_frames - 4, height, width, 3):
            raise ValueError(f"animate_mask_video must be {num_frames - 4} frames (num_frames - 4) of {height}x{width}, "
                             f"got {tuple(m8.shape)}")
        m = (m8[..., 0].float() * (1.0 / 255)).to(self.torch_dtype)    # preprocess_video(max_value=1, min_value=0)
        m = (1 - m.float()).to(self.torch_dtype)                        # :1143, a bf16 tensor op
        return animate_inpaint_y(ref, bg, m)

    def encode_reference_image(self, reference_image, height, width):
        """WanVideoUnit_FunReference's reference_latents (wan_video_new.py:788-790) -> (1, 16, 1, h, w): the
        image resized to (width, height), encoded untiled."""
        if self.vae is None:
            raise RuntimeError("reference_image encoding requires a loaded Wan2.1 VAE (or pass reference_latents=)")
        frame = self._image_frame(reference_image, "reference_image", height, width)
        return self.vae.encode(frame.to(self.torch_dtype), self.device).to(self.torch_dtype)

    def encode_camera_y(self, input_image, num_frames, height, width, tiled=True, tile_size=(30, 52),
                        tile_stride=(15, 26), y=None):
        """WanVideoUnit_FunCameraControl's y (wan_video_new.py:825-844).  in_dim 32: zeros (1, 16, T', h, w)
        with the untiled encode of the input image in latent frame 0; otherwise the mask + latents form of
        the image embedder without an end image (the y __call__ already made from input_image, when given)."""
        dit = self._main_dit()
        if dit.in_dim - 16 != 16:
            return y if y is not None else self.encode_input_image(input_image, None, num_frames, height, width, tiled,
                                                                   tile_size, tile_stride)
        if self.vae is None:
            raise RuntimeError("input_image encoding requires a loaded Wan2.1 VAE")
        frame = self._image_frame(input_image, "input_image", height, width)
        z = self.vae.encode(frame.to(self.torch_dtype), self.device).to(self.torch_dtype)
        out = torch.zeros((1, 16, (num_frames - 1) // 4 + 1, height // 8, width // 8), dtype=self.torch_dtype,
                          device=self.device)
        out[:, :, :1] = z
        return out

    def encode_input_video(self, input_video, input_latents, height, width, num_frames, tiled, tile_size,
                           tile_stride, vace_reference_image=None):
        """WanVideoUnit_InputVideoEmbedder (wan_video_new.py:598-609): preprocess + VAE-encode the
        video (or take its precomputed latents), with the latent of the one reference image, encoded
        untiled, in front along time -> (1, 16, f + T', h, w) bf16 (48 channels at stride 16 with the Wan2.2
        VAE or a DiT of such latents: latent_geometry).  The reference neither truncates
        nor resizes the video here, so a video that does not match the call is an error."""
        from .vae import frames_to_u8, preprocess_video
        t_lat = (num_frames - 1) // 4 + 1
        zc, zs = self.latent_geometry(None if input_video is not None else "latents")   # input_latents: the DiT's
        want = (1, zc, t_lat, height // zs, width // zs)
        refs = None
        if vace_reference_image is not None:
            refs = vace_reference_image              # a list of images, (f, H, W, 3) uint8, or one image
            if not (isinstance(refs, (list, tuple)) or (isinstance(refs, torch.Tensor) and refs.dim() == 4)):
                refs = [refs]
            if len(refs) != 1:
                # :609 concatenates f reference latents as a batch of f onto the batch-1 video latents
                raise ValueError(f"input_video takes exactly one vace_reference_image (got {len(refs)}): the "
                                 "reference pipeline's latent shapes only agree for one")
        if input_video is not None:
            frames = frames_to_u8(input_video, self.device)
            if frames.shape[0] != num_frames:
                raise ValueError(f"input_video has {frames.shape[0]} frames, the call asks for num_frames={num_frames}")
            if tuple(frames.shape[1:3]) != (height, width):
                raise ValueError(f"input_video frames are {frames.shape[1]}x{frames.shape[2]}, the call asks for "
                                 f"{height}x{width}")
        elif tuple(input_latents.shape) != want:
            raise ValueError(f"input_latents must be {want}, got {tuple(input_latents.shape)}")
        if self.vae is None and (input_video is not None or refs is not None):
            raise RuntimeError("input_video encoding requires a loaded VAE (or pass input_latents=)")
        if input_video is not None:
            input_latents = self.vae.encode(preprocess_video(frames), self.device, tiled=tiled, tile_size=tile_size,
                                            tile_stride=tile_stride)
        input_latents = input_latents.to(device=self.device, dtype=self.torch_dtype)
        if refs is not None:
            r = frames_to_u8(refs, self.device)
            if tuple(r.shape[1:3]) != (height, width):
                raise ValueError(f"vace_reference_image must be {height}x{width}, got {r.shape[1]}x{r.shape[2]}")
            ref_latents = self.vae.encode(preprocess_video(r), self.device)             # :608 (untiled)
            input_latents = torch.cat([ref_latents.to(self.torch_dtype), input_latents], dim=2)
        return input_latents.contiguous()

    def encode_vace(self, vace_video, vace_video_mask, height, width, num_frames, tiled, tile_size, tile_stride,
                    vace_reference_image=None):
        """WanVideoUnit_VACE (wan_video_new.py:861-920): 2 tiled VAE encodes + mask latents (+ one
        encode per reference image)."""
        if self.vae is None:
            raise RuntimeError("VACE video encoding requires a loaded Wan2.1 VAE (or pass vace_context=)")
        from .vae import vace_context
        if vace_video is not None and not isinstance(vace_video, torch.Tensor):
            vace_video = list(vace_video)[:num_frames]
        if vace_video_mask is not None and not isinstance(vace_video_mask, torch.Tensor):
            vace_video_mask = list(vace_video_mask)[:num_frames]
        return vace_context(self.vae, vace_video, vace_video_mask, num_frames, height, width, tiled, tile_size,
                            tile_stride, vace_reference_image)

    def vae_output_to_video(self, vae_output, output_type="video"):
        """BasePipeline.vae_output_to_video (utils/__init__.py:76-91): uint8 conversion on the GPU;
        output_type "u8" returns the (T, H, W, 3) uint8 device tensor, "video" PIL images."""
        from .vae import vae_output_to_u8
        u8 = vae_output_to_u8(vae_output[0])
        if output_type == "u8":
            return u8
        from PIL import Image
        return [Image.fromarray(f) for f in u8.cpu().numpy()]
