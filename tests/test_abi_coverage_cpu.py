"""Every compute entry of the C ABI has a direct test.

The names come from vstyler/_lib.py's signature table.  COVERED maps each compute entry to the
`file::test` that calls it directly (through its wrapper or through _lib) and to the name that file
uses for it; EXEMPT lists the host-only entries, each with its reason.  The test fails when an entry
is in neither, when a mapped test function no longer exists in its file, or when that file no longer
names the entry or its wrapper.  Bookkeeping about the suite only: no compiled code is inspected."""
import ast
import os

HERE = os.path.dirname(os.path.abspath(__file__))

# entry -> (file, test function, the name by which the file calls it)
COVERED = {
    "vs_gemm": ("test_kernels_gpu.py", "test_gemm_asymmetric_exact", "K.gemm("),
    "vs_quant_fp8_rows": ("test_fp8_gpu.py", "test_quant_fp8_rows_bit_exact", "quant_fp8_rows("),
    "vs_gemm_fp8": ("test_fp8_gpu.py", "test_gemm_fp8_integer_exact", "gemm_fp8("),
    "vs_gemm_fp8_lora": ("test_fp8_lora_gpu.py", "test_gemm_fp8_lora_integer_exact", "gemm_fp8("),
    "vs_gemm_fp8_ws": ("test_fp8_scaled_gpu.py", "test_gemm_fp8_ws_integer_exact", "scale_w"),
    "vs_attn_fwd": ("test_attention_exact_gpu.py", "test_attention_exact_key_tile_edges", "K.attention("),
    "vs_layernorm_modulate": ("test_kernels_gpu.py", "test_layernorm_modulate_edges", "K.layernorm_modulate("),
    "vs_layernorm_modulate_fp8": ("test_kernels_gpu.py", "test_layernorm_modulate_fp8_edges",
                                  "K.layernorm_modulate_fp8("),
    "vs_residual_layernorm": ("test_kernels_gpu.py", "test_residual_layernorm_edges", "K.residual_layernorm("),
    "vs_rmsnorm_rope": ("test_kernels_gpu.py", "test_rmsnorm_rope_edges", "K.rmsnorm_rope("),
    "vs_patchify": ("test_elementwise_edges_gpu.py", "test_patchify_unpatchify_channels", "K.patchify("),
    "vs_unpatchify": ("test_elementwise_edges_gpu.py", "test_patchify_unpatchify_channels", "K.unpatchify("),
    "vs_cfg_euler": ("test_elementwise_edges_gpu.py", "test_cfg_euler_and_dev", "K.cfg_euler("),
    "vs_cfg_euler_dev": ("test_elementwise_edges_gpu.py", "test_cfg_euler_and_dev", "K.cfg_euler_dev("),
    "vs_time_sinusoid": ("test_elementwise_edges_gpu.py", "test_time_sinusoid_every_timestep", "K.time_sinusoid("),
    "vs_mod_add": ("test_elementwise_edges_gpu.py", "test_mod_add", "K.mod_add("),
    "vs_axpy": ("test_elementwise_edges_gpu.py", "test_axpy", "K.axpy("),
    "vs_ulysses_permute": ("test_elementwise_edges_gpu.py", "test_ulysses_permute_entry", "vs_ulysses_permute"),
    "vs_ulysses_permute_rows": ("test_kernels_gpu.py", "test_ulysses_permute_interleaved_rows", "K.ulysses_permute("),
    "vs_embed_rows": ("test_t5_kernels_gpu.py", "test_embed_rows", "vs_embed_rows"),
    "vs_t5_bias_softmax": ("test_t5_kernels_gpu.py", "test_t5_bias_softmax", "vs_t5_bias_softmax"),
    "vs_t5_gelu_mul": ("test_t5_kernels_gpu.py", "test_t5_gelu_mul_every_bf16", "vs_t5_gelu_mul"),
    "vs_vae_conv": ("test_batched_gemm_gpu.py", "test_batched_gemm_integer_exact", "vae.batched_gemm("),
    "vs_vae_rmsnorm": ("test_vae_gpu.py", "test_rmsnorm_silu_bit_exact", "vae.rmsnorm("),
    "vs_vae_softmax": ("test_vae_helpers_gpu.py", "test_vae_softmax", "vs_vae_softmax"),
    "vs_vae_transpose": ("test_vae_helpers_gpu.py", "test_vae_transpose", "vs_vae_transpose"),
    "vs_vae_attention": ("test_vae_attention_gpu.py", "test_vae_attention_vs_float64", "vs_vae_attention"),
    "vs_vae_tile_gather": ("test_vae_helpers_gpu.py", "test_vae_tile_gather", "vs_vae_tile_gather"),
    "vs_vae_tile_blend": ("test_vae_helpers_gpu.py", "test_vae_tile_blend_and_finish", "vs_vae_tile_blend"),
    "vs_vae_blend_finish": ("test_vae_helpers_gpu.py", "test_vae_tile_blend_and_finish", "vs_vae_blend_finish"),
    "vs_vae_copy_frames": ("test_vae_helpers_gpu.py", "test_vae_copy_frames", "vs_vae_copy_frames"),
    "vs_vae_to_u8": ("test_vae_gpu.py", "test_output_to_u8_bit_exact", "vae_output_to_u8("),
    "vs_unipc_update": ("test_elementwise_edges_gpu.py", "test_unipc_update_modes", "vs_unipc_update"),
    "vs_cast": ("test_elementwise_edges_gpu.py", "test_cast", "vs_cast"),
    "vs_flow_add_noise": ("test_v2v_gpu.py", "test_flow_add_noise_bf16_bit_exact", "flow_add_noise("),
    "vs_vace_prepare": ("test_vace_e2e_gpu.py", "test_vace_prepare_and_mask_latents_bit_exact", "vs_vace_prepare"),
    "vs_vace_mask_latents": ("test_vace_e2e_gpu.py", "test_vace_prepare_and_mask_latents_bit_exact",
                             "vs_vace_mask_latents"),
    "vs_window_blend": ("test_window_gpu.py", "test_window_kernels_bit_exact", "window_blend("),
    "vs_window_finish": ("test_window_gpu.py", "test_window_kernels_bit_exact", "window_finish("),
    "vs_resize_nearest_u8": ("test_experts_gpu.py", "test_resize_nearest_u8_bit_exact", "resize_nearest_u8("),
}

# host-only entries: no device computation to compare
EXEMPT = {
    "vs_abi_version": "returns a constant (test_abi.py)",
    "vs_strerror": "names an error code on the host (test_abi.py)",
    "vs_attn_split_plan": "host-only plan arithmetic (test_abi.py::test_attention_split_plan_host_only)",
    "vs_gemm_split_plan": "host-only plan arithmetic (test_abi.py::test_gemm_split_plan_host_only)",
    "vs_gemm_route": "host-only route query (test_abi.py::test_gemm_route_is_fused_everywhere)",
    "vs_gemm_route_epi": "host-only route query (test_abi.py::test_gemm_route_is_fused_everywhere)",
    "vs_split_workspace_bytes": "host-only size query",
    "vs_split_workspace_bind": "registers a caller-owned buffer on the host; launches nothing",
    "vs_set_option": "host-side option table (test_abi.py::test_options_table)",
    "vs_get_option": "host-side option table (test_abi.py::test_options_table)",
    "vs_sp_unique_id": "RCCL bootstrap on the host (test_sp.py)",
    "vs_sp_init": "RCCL communicator setup (test_sp.py)",
    "vs_sp_all_to_all": "an RCCL collective, no kernel of this library (test_sp.py)",
    "vs_sp_all_gather": "an RCCL collective, no kernel of this library (test_sp.py)",
    "vs_sp_comm_destroy": "RCCL communicator teardown (test_sp.py)",
    "vs_sp_last_error": "host-side error text (test_sp.py)",
}


def _entries():
    from vstyler import _lib
    return set(_lib.SIGNATURES)


def _test_functions(path):
    with open(path) as f:
        tree = ast.parse(f.read())
    return {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}


def test_every_entry_is_covered_or_exempt():
    entries = _entries()
    both = set(COVERED) & set(EXEMPT)
    assert not both, f"listed as covered and exempt: {sorted(both)}"
    missing = entries - set(COVERED) - set(EXEMPT)
    assert not missing, f"ABI entries without a direct test (add one, then map it here): {sorted(missing)}"
    stale = (set(COVERED) | set(EXEMPT)) - entries
    assert not stale, f"not in vstyler/_lib.py's signature table any more: {sorted(stale)}"
    assert all(reason.strip() for reason in EXEMPT.values())


def test_mapped_tests_exist_and_name_their_entry():
    problems = []
    funcs, texts = {}, {}
    for entry, (fname, test, needle) in sorted(COVERED.items()):
        path = os.path.join(HERE, fname)
        if fname not in funcs:
            if not os.path.exists(path):
                problems.append(f"{entry}: {fname} does not exist")
                continue
            funcs[fname] = _test_functions(path)
            with open(path) as f:
                texts[fname] = f.read()
        if test not in funcs[fname]:
            problems.append(f"{entry}: {fname} has no function {test}")
        if needle not in texts[fname] and entry not in texts[fname]:
            problems.append(f"{entry}: {fname} names neither {needle!r} nor {entry}")
    assert not problems, "\n".join(problems)
