"""Image-to-video on the GPU: the image cross-attention block, the tiny forward with y / clip_feature
against tests/i2v_util.py within the oracle's floor, the bit-identity checks (fused == unfused route, CFG
batch == two batch-1 forwards, in_dim 16 untouched), the 2-step Euler loops (eager, hipGraph, two experts,
sliding window) against test-side loops, and the pipeline with a tiny VAE against its steps done by hand.

Tiny model: dim 256, 2 heads, 2 layers, in_dim 36; latents (1, 16, 3, 8, 12): S = 72 tokens."""
import pytest
import torch

import i2v_util as I
from gpu_util import err
from oracle import wan_oracle as O
from oracle import wan_vae_oracle as V
from vae_util import TINY_VAE

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
H, WD = 64, 96


def bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def within_floor(got, ref, ref64, tag):
    """The oracle-floor rule of tests/test_experts_gpu.py: the floor is the restatement accumulating in
    float64 against the float32 one."""
    fmx, frel = err(ref64, ref)
    mx, rel = err(got, ref)
    print(f"{tag}: max-abs {mx:.4g} rel-L2 {rel:.4g} (floor {fmx:.4g} / {frel:.4g})")
    assert rel <= 1.5 * frel + 2e-3 and mx <= 1.5 * fmx + 2e-2, (tag, mx, rel, fmx, frel)


VARIANTS = {"y": dict(has_image_input=False), "y+clip": dict(has_image_input=True),
            "y+clip514": dict(has_image_input=True, has_image_pos_emb=True)}


@pytest.fixture(scope="module")
def models():
    """Per variant: (cfg, W, dit, (lat, y, clip, cp, cn), ref, ref64) -- the references computed once."""
    out = {}
    for name, flags in VARIANTS.items():
        cfg = I.tiny_cfg(**flags)
        W = I.random_weights(cfg, seed=5)
        dit = I.build(cfg, W)
        lat, y, clip, cp, cn = I.inputs(cfg, clip_rows=514 if flags.get("has_image_pos_emb") else 257)
        if not flags["has_image_input"]:
            clip = None
        t = torch.tensor([700.0]).to(BF16)

        def run():
            return I.model_fn(W, cfg, lat, t, cp, y, clip)
        out[name] = (cfg, W, dit, (lat, y, clip, cp, cn), run(), I.with_float64(run))
    return out


def fwd(dit, lat, ctx, y, clip, t=700.0, **kw):
    from vstyler import model_fn_wan_video
    return model_fn_wan_video(dit, latents=lat.cuda(), timestep=torch.tensor([t]).to(BF16).cuda(), context=ctx.cuda(),
                              y=None if y is None else y.cuda(), clip_feature=None if clip is None else clip.cuda(),
                              **kw)


# --------------------------------------------------------------------------------------- single forwards
def test_dit_block_image_branch(models):
    """One DiTBlock with the image branch (fused route) on embedded rows, against i2v_util.dit_block."""
    from vstyler.models import RunCtx, Workspace
    from vstyler.options import host_options
    cfg, W, dit, _, _, _ = models["y+clip"]
    D, Hh, L, grid = cfg["dim"], cfg["num_heads"], 64, (3, 4, 6)
    S = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(21)
    x = torch.randn((1, S, D), generator=g).to(BF16)
    ctx = torch.randn((1, L, D), generator=g).to(BF16)
    img = torch.randn((1, 257, D), generator=g).to(BF16)
    t_mod = (0.1 * torch.randn((1, 6, D), generator=g)).to(BF16)
    freqs = O.rope_freqs(*grid, D // Hh)

    def run():
        return I.dit_block(x, torch.cat([img, ctx], dim=1), t_mod, freqs, W, "blocks.0.", Hh, True)
    ref, ref64 = run(), I.with_float64(run)
    rc = RunCtx(1, S, grid, dit.rope("cuda"), ctx.cuda().view(L, D), L, Workspace("cuda"))
    rc.img, rc.img_batch = img.cuda().view(257, D), 1
    xd = x.cuda().view(S, D).clone()
    with host_options(img_attn_fused=1):
        dit.blocks[0](xd, t_mod.cuda(), rc)
    torch.cuda.synchronize()
    assert not torch.equal(xd.cpu(), x.view(S, D))
    within_floor(xd.view(1, S, D), ref, ref64, "DiTBlock with image branch")
    # without the image rows the block refuses to run (no silent text-only attention)
    rc.img = None
    with pytest.raises(ValueError, match="clip_feature"):
        dit.blocks[0](x.cuda().view(S, D).clone(), t_mod.cuda(), rc)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_tiny_forward_vs_i2v_util(models, variant):
    cfg, W, dit, (lat, y, clip, cp, cn), ref, ref64 = models[variant]
    got = fwd(dit, lat, cp, y, clip)
    torch.cuda.synchronize()
    assert got.shape == (1, 16, 3, 8, 12)
    within_floor(got, ref, ref64, f"tiny forward [{variant}]")
    # the conditioning reaches the output: another y / another clip_feature changes it
    assert not torch.equal(fwd(dit, lat, cp, torch.zeros_like(y), clip), got)
    if clip is not None:
        assert not torch.equal(fwd(dit, lat, cp, y, torch.roll(clip, 1, dims=2)), got)


# -------------------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize("variant", ["y+clip", "y+clip514"])
def test_fused_route_equals_unfused_route(models, variant):
    """The CFG forward with the image attention added inside vs_attn_fwd_add == the same forward with
    K.attention into a scratch buffer + K.axpy, bit for bit, the unfused image attention on the checked
    8-wave kernel (attn_nc=0, attn_impl=8).  Both forwards run under those options: they also select the
    kernel of the self- and text attention, whose optimistic (NC) results are not the checked kernel's
    bits (first run with the fused forward under the default options: the outputs differed in the last
    place through those attentions); vs_attn_fwd_add itself reads neither option."""
    from vstyler import kernels as K
    from vstyler.options import host_options
    cfg, W, dit, (lat, y, clip, cp, cn), _, _ = models[variant]
    both = torch.cat([cp, cn])
    with K.options(attn_nc=0, attn_impl=8):
        with host_options(img_attn_fused=1):
            fused = fwd(dit, lat, both, y, clip).clone()
        with host_options(img_attn_fused=0):
            unfused = fwd(dit, lat, both, y, clip).clone()
    assert torch.equal(bits(fused), bits(unfused))


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_cfg_batch_equals_two_single_forwards(models, variant, fused):
    """B = 2 (shared latents / y / clip_feature: the shared prefix applies) == two batch-1 forwards, with
    cfg_prefix on and off; and with a per-sample y (no shared prefix) likewise."""
    from vstyler import kernels as K
    from vstyler.options import host_options
    cfg, W, dit, (lat, y, clip, cp, cn), _, _ = models[variant]
    with host_options(img_attn_fused=fused), K.options(gemm_split=0, attn_split=0, attn_nc=0, attn_impl=8):
        one = torch.cat([fwd(dit, lat, cp, y, clip).clone(), fwd(dit, lat, cn, y, clip).clone()])
        for prefix in (1, 0):
            with host_options(cfg_prefix=prefix):
                two = fwd(dit, lat, torch.cat([cp, cn]), y, clip).clone()
            assert torch.equal(bits(two), bits(one)), prefix
        y2 = torch.cat([y, torch.flip(y, dims=(2,))])
        c2 = None if clip is None else torch.cat([clip, torch.roll(clip, 1, dims=2)])
        per = fwd(dit, lat, torch.cat([cp, cn]), y2, c2).clone()
        other = fwd(dit, lat, cn, y2[1:], None if c2 is None else c2[1:]).clone()
        assert torch.equal(bits(per[0:1]), bits(one[0:1])) and torch.equal(bits(per[1:2]), bits(other))


def test_in_dim_16_takes_the_old_path(monkeypatch):
    """A 16-channel model runs the calls it ran before image conditioning: vs_patchify + one GEMM on the
    unpadded weight (restated here from the previous PatchEmbed.forward), never the new kernels."""
    from vstyler import kernels as K
    from vstyler import model_fn_wan_video
    from vstyler.models import PatchEmbed
    from test_model_gpu import build
    cfg = O.WAN_CONFIGS["tiny"]
    W = O.random_weights(cfg, seed=5)
    dit, vace = build(cfg, W)
    lat, cp, cn, vc = O.synthetic_inputs(cfg, 5, 64, 96)
    t = torch.tensor([1000.0]).to(BF16).cuda()
    for name in ("patchify2", "attention_add", "gelu_erf"):
        monkeypatch.setattr(K, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("new kernel on the old path")))
    got = model_fn_wan_video(dit, vace=vace, latents=lat.cuda(), timestep=t, context=torch.cat([cp, cn]).cuda(),
                             vace_context=vc.cuda()).clone()

    def previous(self, lat, ws, tag):
        B, C, T, Hh, Ww = lat.shape
        S = T * (Hh // 2) * (Ww // 2)
        cols = ws.get(tag + ".cols", (B * S, C * 4))
        K.patchify(lat.contiguous(), cols)
        out = ws.get(tag + ".out", (B * S, self.dim))
        K.gemm(cols, self.weight.view(self.dim, C * 4), out, bias=self.bias)
        return out, (T, Hh // 2, Ww // 2)
    monkeypatch.setattr(PatchEmbed, "forward", previous)
    want = model_fn_wan_video(dit, vace=vace, latents=lat.cuda(), timestep=t, context=torch.cat([cp, cn]).cuda(),
                              vace_context=vc.cuda())
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------ Euler loops
def euler_loop(dits, lat, cp, cn, y, clip, steps=2, boundary=0.875, **fwd_kw):
    """The test-side loop around model_fn_wan_video (tests/test_experts_gpu.py euler_loop, with y /
    clip_feature): expert 2 iff the fp32 timestep is below boundary * 1000."""
    from vstyler import kernels as K
    from vstyler import model_fn_wan_video
    from vstyler.flow_match import FlowMatchScheduler
    sch = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(steps, denoising_strength=1.0, shift=5.0)
    x = lat.cuda().to(BF16).contiguous().clone()
    both = torch.cat([cp, cn]).cuda()
    for i, t in enumerate(sch.timesteps):
        dit = dits[1] if len(dits) > 1 and float(t) < boundary * 1000 else dits[0]
        v = model_fn_wan_video(dit, latents=x, timestep=t.reshape(1).to(BF16).cuda(), context=both, y=y.cuda(),
                               clip_feature=None if clip is None else clip.cuda(), **fwd_kw)
        d = torch.tensor([sch.delta(i)], dtype=torch.float32, device="cuda")
        K.cfg_euler_dev(v[0:1], v[1:2], x, 5.0, d)
    return x


def oracle_chain(Ws, cfg, lat, cp, cn, y, clip, steps=2, boundary=875.0):
    sigmas, timesteps = O.set_timesteps(steps, 1.0, 5.0)
    x = lat
    for i, ts in enumerate(timesteps):
        W = Ws[1] if len(Ws) > 1 and float(ts) < boundary else Ws[0]
        t = ts.unsqueeze(0).to(BF16)
        vp = I.model_fn(W, cfg, x, t, cp, y, clip)
        vn = I.model_fn(W, cfg, x, t, cn, y, clip)
        x = O.cfg_euler(vp, vn, x, 5.0, O.euler_delta(sigmas, i))
    return x


@pytest.fixture(scope="module")
def pipe2(models):
    """A pipeline with the y+clip model as dit and a second expert of other weights (seed 6)."""
    from vstyler import WanVideoPipeline
    cfg, W, dit, inp, _, _ = models["y+clip"]
    W2 = I.random_weights(cfg, seed=6)
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit = dit
    return pipe, cfg, (W, W2), I.build(cfg, W2), inp


def _denoise(pipe, lat, cp, cn, y, clip, **kw):
    return pipe.denoise(lat, cp.cuda(), cn.cuda(), num_inference_steps=2, y=y, clip_feature=clip, **kw)


def test_euler_loop_eager_and_graph(pipe2):
    pipe, cfg, (W, W2), dit2, (lat, y, clip, cp, cn) = pipe2
    want = euler_loop([pipe.dit], lat, cp, cn, y, clip)
    eager = _denoise(pipe, lat, cp, cn, y, clip, use_graph=False)
    assert pipe.last_graph is None
    graph = _denoise(pipe, lat, cp, cn, y, clip, use_graph=True)
    assert pipe.last_graph is not None
    assert torch.equal(bits(eager), bits(want)) and torch.equal(bits(graph), bits(want))

    def chain():
        return oracle_chain([W], cfg, lat, cp, cn, y, clip)
    within_floor(graph, chain(), I.with_float64(chain), "euler 2 steps, y + clip_feature")


def test_euler_loop_two_experts(pipe2):
    """2 steps, shift 5: timesteps 1000, 833.3 -- the boundary 0.875 switches to dit2 for the second."""
    pipe, cfg, (W, W2), dit2, (lat, y, clip, cp, cn) = pipe2
    pipe.dit2 = dit2
    try:
        want = euler_loop([pipe.dit, dit2], lat, cp, cn, y, clip)
        eager = _denoise(pipe, lat, cp, cn, y, clip, use_graph=False)
        graph = _denoise(pipe, lat, cp, cn, y, clip, use_graph=True)
    finally:
        pipe.dit2 = None
    one = _denoise(pipe, lat, cp, cn, y, clip, use_graph=False)
    assert torch.equal(bits(eager), bits(want)) and torch.equal(bits(graph), bits(want))
    assert not torch.equal(bits(one), bits(want)), "dit2 was ignored"

    def chain():
        return oracle_chain([W, W2], cfg, lat, cp, cn, y, clip)
    within_floor(graph, chain(), I.with_float64(chain), "euler 2 steps, two experts")


def test_euler_loop_sliding_window(pipe2):
    """sliding_window_size 2, stride 1 over T = 3: the product's windowed step equals the test-side tiler
    (window_util.tile's arithmetic) that cuts y with the latents, eager and captured."""
    from vstyler import model_fn_wan_video
    pipe, cfg, (W, W2), dit2, (lat, y, clip, cp, cn) = pipe2

    def tiled(dit, latents=None, y=None, **kw):
        return I.tile_y(lambda lw, yw: model_fn_wan_video(dit, latents=lw.contiguous(), y=yw.contiguous(), **kw),
                        latents, y, 2, 1)
    from vstyler import kernels as K
    from vstyler.flow_match import FlowMatchScheduler
    sch = FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(2, denoising_strength=1.0, shift=5.0)
    x = lat.cuda().clone()
    both = torch.cat([cp, cn]).cuda()
    for i, t in enumerate(sch.timesteps):
        v = tiled(pipe.dit, latents=x, y=y.cuda(), timestep=t.reshape(1).to(BF16).cuda(), context=both,
                  clip_feature=clip.cuda())
        K.cfg_euler_dev(v[0:1], v[1:2], x, 5.0, torch.tensor([sch.delta(i)], dtype=torch.float32, device="cuda"))
    kw = dict(sliding_window_size=2, sliding_window_stride=1)
    eager = _denoise(pipe, lat, cp, cn, y, clip, use_graph=False, **kw)
    graph = _denoise(pipe, lat, cp, cn, y, clip, use_graph=True, **kw)
    assert torch.equal(bits(eager), bits(x)) and torch.equal(bits(graph), bits(x))
    assert not torch.equal(bits(eager), bits(_denoise(pipe, lat, cp, cn, y, clip, use_graph=False)))


# ------------------------------------------------------------------------------------------- pipeline
def test_pipeline_input_image_end_image(models):
    """pipe(prompt_emb=..., input_image=, end_image=, output_type="latents") against its steps done by hand:
    encode_input_image, then denoise; and y's layout: 4 mask channels (first and last latent frame known)
    over the VAE latents of [image, zeros, end_image] (the reference's lines restated in i2v_util)."""
    from vstyler import WanVideoPipeline, vae
    cfg, W, dit, (lat, _, _, cp, cn), _, _ = models["y"]
    Wv = V.random_vae_weights(TINY_VAE, seed=34)
    pipe = WanVideoPipeline(device="cuda")
    pipe.dit = dit
    pipe.vae = vae.WanVideoVAE(z_dim=16, dim=TINY_VAE["dim"], device="cuda").load_state_dict(Wv)
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (H, WD, 3), generator=g, dtype=torch.uint8)
    img2 = torch.randint(0, 256, (H, WD, 3), generator=g, dtype=torch.uint8)
    nf, ts, st = 9, (4, 6), (2, 3)
    kw = dict(height=H, width=WD, num_frames=nf, num_inference_steps=2, seed=3, tile_size=ts, tile_stride=st)
    got = pipe(prompt_emb=cp, negative_prompt_emb=cn, input_image=img.numpy(), end_image=img2, output_type="latents",
               **kw)
    y = pipe.encode_input_image(img, img2, nf, H, WD, True, ts, st)
    assert y.shape == (1, 20, 3, H // 8, WD // 8) and y.dtype == BF16
    noise = pipe.generate_noise((1, 16, 3, H // 8, WD // 8), seed=3)
    want = pipe.denoise(noise, cp.cuda(), cn.cuda(), num_inference_steps=2, y=y)
    assert torch.equal(bits(got), bits(want))
    # the layout of y against the reference's lines restated (i2v_util)
    pre = [V.preprocess_video(f[None]) for f in (img, img2)]                      # (1, 3, 1, H, W)
    msk, vin = I.reference_mask_and_vae_input(pre[0][0].transpose(0, 1), pre[1][0].transpose(0, 1), nf, H, WD)
    assert torch.equal(y[0, :4].float().cpu(), msk)
    enc = pipe.vae.encode(vin[None].to(BF16).cuda(), "cuda", tiled=True, tile_size=ts, tile_stride=st)
    assert torch.equal(bits(y[:, 4:]), bits(enc))
    # without end_image the last latent frame is unknown, and the result differs
    y1 = pipe.encode_input_image(img, None, nf, H, WD, True, ts, st)
    assert float(y1[0, :4, -1].abs().max()) == 0 and float(y1[0, :4, 0].min()) == 1
    assert not torch.equal(bits(pipe(prompt_emb=cp, negative_prompt_emb=cn, input_image=img, output_type="latents",
                                     **kw)), bits(got))


# -------------------------------------------------------------------------------------------- Ulysses
def _ulysses_worker(rank, world, port, q):
    try:
        from test_sp import _init
        _init(rank, world, port)
        from sp_util import HostStagedUlysses
        from vstyler import model_fn_wan_video
        cfg = I.tiny_cfg(has_image_input=True)
        dit = I.build(cfg, I.random_weights(cfg, seed=5), "cuda:0")
        lat, y, clip, cp, cn = I.inputs(cfg)
        kw = dict(latents=lat.cuda(), timestep=torch.tensor([700.0]).to(BF16).cuda(), context=torch.cat([cp, cn]).cuda(),
                  y=y.cuda(), clip_feature=clip.cuda())
        single = model_fn_wan_video(dit, **kw)
        res = {}
        for overlap in (True, False):
            sp = HostStagedUlysses()
            sp.overlap = overlap
            par = model_fn_wan_video(dit, use_unified_sequence_parallel=True, sp_group=sp, **kw)
            torch.cuda.synchronize()
            res[f"overlap{int(overlap)}"] = torch.equal(single.cpu(), par.cpu())
        q.put((rank, res))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def test_ulysses_world2_equals_single_gpu():
    """Everything image conditioning adds is token-local: the world-2 Ulysses forward with y + clip_feature
    (tests/sp_util.py's host-staged group, both ranks on one GPU) equals the single-GPU forward bit for
    bit, under both micro-batch schedules."""
    from test_sp import _spawn
    res = _spawn(_ulysses_worker, 2, timeout=300)
    assert len(res) == 2
    for rank, r in res:
        assert isinstance(r, dict), res
        assert r["overlap1"] is True and r["overlap0"] is True, (rank, r)


# ------------------------------------------------------------------------------- LoRA and fp8 around it
def test_lora_and_fp8_leave_the_image_projections_working(models):
    """merge_lora reaches k_img through the generic name map and the fused k_img | v_img GEMM sees the
    merged weight (the forward equals that of a model loaded with the merged weight); a hot-loaded
    adapter on v_img un-fuses the pair and gives the merged model's output up to the rounding of the
    merged bf16 weight (rel-L2 < 1e-2, the project's forward-parity level); quantize_fp8_ converts the
    block Linears only and the forward still runs."""
    from vstyler.lora import hotload_lora, merge_lora
    from vstyler.models import fused_img_linear, quantize_fp8_, Workspace
    cfg, W, _, (lat, y, clip, cp, cn), _, _ = models["y+clip"]
    D = cfg["dim"]
    g = torch.Generator().manual_seed(9)
    lora = {}
    for name in ("blocks.0.cross_attn.k_img", "blocks.1.cross_attn.v_img"):
        lora[name + ".lora_A.default.weight"] = (0.1 * torch.randn((8, D), generator=g)).to(BF16)
        lora[name + ".lora_B.default.weight"] = (0.1 * torch.randn((D, 8), generator=g)).to(BF16)
    base = fwd(I.build(cfg, W), lat, cp, y, clip).clone()
    merged = I.build(cfg, W)
    assert merge_lora(merged, lora, alpha=1.0) == 2
    sd = {k: v.clone() for k, v in merged.state_dict().items()}
    k = "blocks.0.cross_attn.k_img.weight"
    want = W[k].float() + lora["blocks.0.cross_attn.k_img.lora_B.default.weight"].float() @ \
        lora["blocks.0.cross_attn.k_img.lora_A.default.weight"].float()
    assert not torch.equal(sd[k].cpu(), W[k]) and float((sd[k].cpu().float() - want).abs().max()) < 2e-3
    ca = merged.blocks[0].cross_attn
    assert fused_img_linear(ca, torch.zeros(257, D, dtype=BF16, device="cuda"), Workspace("cuda"), "t") is not None
    out_m = fwd(merged, lat, cp, y, clip).clone()
    assert not torch.equal(bits(out_m), bits(base))
    assert torch.equal(bits(fwd(I.build(cfg, {k: v.cpu() for k, v in sd.items()}), lat, cp, y, clip)), bits(out_m))
    hot = I.build(cfg, W)
    assert hotload_lora(hot, lora, alpha=1.0) == 2
    assert fused_img_linear(hot.blocks[0].cross_attn, torch.zeros(257, D, dtype=BF16, device="cuda"),
                            Workspace("cuda"), "t") is None
    out_h = fwd(hot, lat, cp, y, clip).clone()
    mx, rel = err(out_h, out_m)
    print(f"hot-loaded vs merged LoRA on k_img / v_img: max-abs {mx:.4g} rel-L2 {rel:.4g}")
    assert rel < 1e-2
    q8 = I.build(cfg, W)
    n = quantize_fp8_(q8, weight_scale="channel")
    assert n == 10 * cfg["num_layers"]
    for blk in q8.blocks:
        for lin in (blk.cross_attn.k_img, blk.cross_attn.v_img):
            assert getattr(lin, "weight_fp8", None) is None
    out8 = fwd(q8, lat, cp, y, clip)
    mx, rel = err(out8, base)
    print(f"fp8 block linears, bf16 image branch vs bf16: max-abs {mx:.4g} rel-L2 {rel:.4g}")
    assert torch.isfinite(out8.float()).all() and not torch.equal(bits(out8), bits(base))
