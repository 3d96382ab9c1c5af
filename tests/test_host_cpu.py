"""CPU-side checks of the product's host logic (no kernel launches): C-ABI exports, config/bucket logic, flat
parameter layout, scheduler tables vs the oracle, forward-ordered specs vs the oracle's parameter trees."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import nets as onets
from oracle import schedulers as osched
from stable_diffusion_training_amd import _lib, nets, params, schedulers, training_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "sdt.h")).read()
    declared = set(re.findall(r"\b(sdt_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 38
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/sdt.h but not exported"
    bound = set(_lib.SIGNATURES) | set(_lib.NOARG) | set(_lib.WS_QUERY)
    assert declared == bound, f"binding table out of sync: {declared ^ bound}"
    assert lib.sdt_abi_version() == 5


def test_argument_validation_without_gpu(lib):
    # invalid-arg paths return before any HIP call, so they are checkable on a CPU-only box
    assert lib.sdt_sqnorm_accumulate(None, 0, None, None, 0, None) == -1
    assert b"null pointer" in lib.sdt_last_error()
    assert lib.sdt_lion8_step(1, 1, 0, 1, 1, None, None, 17, 16, None, 1, 1.0, 1e-6, 0.0, 0.9, 0.99, 0.0, None) == -1
    assert b"multiple of block_size" in lib.sdt_last_error()
    assert lib.sdt_lion8_step(16, 8, 0, 16, 16, None, None, 16, 16, None, 16, 1.0, 1e-6, 0.0, 0.9, 0.99, 0.0, None) == -1  # fp32 gradient: 16-byte aligned
    assert b"misaligned" in lib.sdt_last_error()
    assert lib.sdt_sqnorm_accumulate_bf16(None, 0, None, None, 0, None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert lib.sdt_gemm_nt_bf16(16, 16, 16, None, None, None, 4, 12, 8, 1, 8, 8, 0, 8, 0, 0, 0, None, None, 0, None, 0, 0, 0, 0, 0, None) == -1
    assert b"multiples of 8" in lib.sdt_last_error()
    # a row-bias pitch without a row bias, or narrower than the output, is refused (ld_rowbias: column slices of a grouped projection)
    assert lib.sdt_gemm_nt_bf16(16, 16, 16, None, None, None, 8, 16, 8, 1, 8, 8, 0, 16, 0, 0, 0, None, None, 0, None, 0, 0, 0, 0, 48, None) == -1
    assert b"ld_rowbias" in lib.sdt_last_error()
    assert lib.sdt_gemm_nt_bf16(16, 16, 16, None, 16, None, 8, 16, 8, 1, 8, 8, 0, 16, 0, 4, 0, None, None, 0, None, 0, 0, 0, 0, 8, None) == -1
    assert b"ld_rowbias" in lib.sdt_last_error()
    with pytest.raises(_lib.SdtError):
        _lib.call("sdt_geglu_fwd", 16, 16, 4, 12, None)


def test_planner_queries_of_the_round_three_paths(lib):
    """Host-side answers that involve no launch: which feed-forward shapes the GEGLU epilogue serves, the slot count of the fused
    gradient-norm partials, and their argument checks."""
    # SD1.5 / SDXL feed-forward shapes at batch 4 are served; a 300-row one (64-tiles) and a gated width that is no multiple of 64 are not
    for M, C in ((16384, 320), (4096, 640), (1024, 1280)):
        assert lib.sdt_ff_geglu_supported(M, 4 * C, C) == 1
    assert lib.sdt_ff_geglu_supported(300, 256, 64) == 0 and lib.sdt_ff_geglu_supported(16384, 1000, 320) == 0
    assert lib.sdt_ff_geglu_fwd(None, None, None, None, None, 16384, 1280, 320, None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert lib.sdt_ff_geglu_fwd(16, 16, None, 16, 16, 300, 256, 64, None) == -1 and b"not served" in lib.sdt_last_error()
    # 32 x 32 blocks over whole 128-tiles, per tap
    assert lib.sdt_wgrad_sq_slots(320, 320, 1) == 12 * 12 and lib.sdt_wgrad_sq_slots(1280, 640, 9) == 9 * 40 * 20
    assert lib.sdt_wgrad_sq_slots(0, 8, 1) == 0
    assert lib.sdt_sum_f64_accumulate(None, 4, None, None, 0, None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert lib.sdt_stream_wait_event_external is not None


def _dynamic_imports(path):
    """Names of the undefined (imported) symbols in the .dynsym table of a 64-bit little-endian ELF shared object."""
    import struct
    blob = open(path, "rb").read()
    assert blob[:4] == b"\x7fELF" and blob[4] == 2 and blob[5] == 1, "expected a 64-bit little-endian ELF file"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, sh_type, _, _, off, size, link, _, _, entsize in sections:
        if sh_type != 11:  # SHT_DYNSYM
            continue
        str_off = sections[link][4]
        for k in range(size // entsize):
            st_name, _, _, st_shndx = struct.unpack_from("<IBBH", blob, off + k * entsize)
            if st_shndx == 0 and st_name:  # SHN_UNDEF
                names.add(blob[str_off + st_name: blob.index(b"\0", str_off + st_name)].decode())
    return names


def test_default_build_has_no_wrong_result_switches(lib):
    """The library reads no environment variable: planning is a function of the problem shape alone, and the timing ablations
    (kernels that skip waits / math / stores) and the measured-slower 16x16x32 halo variant are gone, so no stray environment
    variable can change a result or corrupt a training run."""
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"SDT_NT_DBG", b"SDT_ATTN_DBG", b"SDT_HALO_MFMA", b"SDT_HALO_BN",
                 b"SDT_NT_SPLIT_WG1", b"SDT_NT_SPLIT_WG2", b"SDT_NT_SPLIT_STEPS1", b"SDT_NT_SPLIT_STEPS2", b"SDT_NT_SPLIT_MINT1",
                 b"SDT_NT_SPLIT_MAXT1", b"SDT_NT_TM", b"SDT_NT_DEEP_RING", b"SDT_NT_NFAST", b"SDT_NT_K32_STEPS",
                 b"SDT_WGRAD3", b"SDT_WGRAD3_MIN_M", b"SDT_WGRAD3_WG", b"SDT_WGRAD3_MIN_ROWS", b"SDT_TN_TM", b"SDT_TN_TARGET_WG",
                 b"SDT_TN_MIN_ROWS", b"SDT_TN_GROUP_WG", b"SDT_TN_WG_FIXED_STEPS",
                 b"SDT_CONV_HALO", b"SDT_CONV_HALO_MINPX", b"SDT_CONV_HALO_WG"):
        assert name not in blob, f"{name.decode()} is readable by the default build"
    imports = _dynamic_imports(_lib.LIB_PATH)
    assert any(n.startswith("hip") for n in imports), "no HIP imports found: bad ELF parse"
    assert not {"getenv", "secure_getenv"} & imports, "the library imports getenv"


def test_no_cpu_fallback_when_no_device(lib):
    if lib.sdt_device_count() == 0:
        with pytest.raises(_lib.SdtError, match="no HIP device"):
            _lib.require_device()


def test_resolution_buckets_kat():
    r = training_utils.calculate_resolution_array(512 ** 2, 256, 64).tolist()
    assert r == [[256, 1024], [320, 768], [384, 640], [448, 576], [512, 512], [576, 448], [640, 384], [768, 320], [1024, 256]]
    assert training_utils.calculate_resolution_array(512 ** 2, 512).tolist() == [[512, 512]]
    example = json.load(open(os.path.join(ROOT, "tests", "golden", "model_properties_keys.json")))
    n = sum(len(training_utils.calculate_resolution_array(a ** 2, m, 64)) for a, m in
            zip(example["image_area_root"], example["minimum_axis_length"]))
    assert n == 41  # the example config compiles 41 programs


def test_training_config_from_dict_picks_28_fields():
    example = json.load(open(os.path.join(ROOT, "tests", "golden", "model_properties_keys.json")))
    cfg = training_utils.TrainingConfig.from_dict(example)
    assert len(cfg.__dataclass_fields__) == 28 and cfg.quant_block_size == 16 and cfg.prediction_type == "v_prediction"


def test_create_mask_semantics():
    m = params.create_mask(["conv_in/kernel", "d/conv_input/kernel", "a/b/bias"], ["conv_in", "bias"])
    assert m == {"conv_in/kernel": False, "d/conv_input/kernel": True, "a/b/bias": False}


@pytest.mark.parametrize("name", ["tiny", "sd15", "sd21", "sdxl"])
def test_unet_spec_matches_oracle_tree(name):
    spec = nets.unet_spec(nets.unet_config(name))
    assert dict(spec) == {k: tuple(v) for k, v in onets.unet_param_shapes(onets.unet_config(name)).items()}
    assert len(spec) == len(dict(spec))


@pytest.mark.parametrize("name", ["tiny", "sd15", "sdxl"])
def test_unet_spec_groups_shared_input_projections(name):
    """unet_spec lays the Dense layers that read one tensor in every block - time_emb_proj (silu(temb)) and attn2 to_k / to_v (the
    text context) - back to back per output width so ops.linear_multi can run a width as one GEMM: kernels adjacent (k, v
    interleaved per block), biases adjacent, the group at the position of its first member, nothing else reordered."""
    spec = nets.unet_spec(nets.unet_config(name))
    names = [n for n, _ in spec]
    shapes = dict(spec)
    pos = {n: i for i, n in enumerate(names)}
    for suffix, step in (("/time_emb_proj/kernel", 1), ("/attn2/to_k/kernel", 2)):
        by_width = {}
        for n in names:
            if n.endswith(suffix):
                by_width.setdefault(shapes[n][1], []).append(n)
        assert by_width
        for width, members in by_width.items():
            idx = [pos[m] for m in members]
            assert idx == list(range(idx[0], idx[0] + step * len(idx), step)), (name, suffix, width)  # back to back, in forward order
            if step == 2:  # to_v of a block right behind its to_k
                assert all(names[i + 1] == m.replace("/to_k/", "/to_v/") for i, m in zip(idx, members))
            else:          # biases follow the kernels of the group, same order
                b0 = idx[-1] + 1
                assert [names[b0 + j] for j in range(len(members))] == [m.replace("/kernel", "/bias") for m in members]
            # the group sits where its first member was declared: directly behind that block's preceding leaf
            first = members[0]
            prev = names[idx[0] - 1]
            block = first[: first.index(suffix.split("/")[1]) - 1]
            assert prev.startswith(block.rsplit("/", 1)[0] if step == 2 else block), (prev, first)
    # everything else keeps the forward order of the ungrouped tree (the oracle's)
    rest = [n for n in names if "/time_emb_proj/" not in n and "/attn2/to_k/" not in n and "/attn2/to_v/" not in n]
    ref = [n for n in onets.unet_param_shapes(onets.unet_config(name)) if "/time_emb_proj/" not in n and "/attn2/to_k/" not in n and "/attn2/to_v/" not in n]
    assert sorted(rest) == sorted(ref)


def test_vae_clip_specs_match_oracle_trees():
    assert dict(nets.vae_encoder_spec(nets.vae_config("sd"))) == onets.vae_encoder_param_shapes(onets.vae_config("sd"))
    assert dict(nets.clip_text_spec(nets.clip_config("clip_l"))) == onets.clip_param_shapes(onets.clip_config("clip_l"))


@pytest.mark.parametrize("sched", ["linear", "scaled_linear", "zero_snr_scaled_linear", "squaredcos_cap_v2"])
def test_scheduler_tables_bit_exact_vs_oracle(sched):
    s = schedulers.DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule=sched, num_train_timesteps=1000)
    st = s.create_state("cpu")
    ref = osched.create_state(sched)
    for k in ("alphas", "betas", "alphas_cumprod"):
        assert np.array_equal(getattr(st, k).numpy(), ref[k], equal_nan=True), k
    with pytest.raises(NotImplementedError):
        schedulers.DDPMScheduler(beta_schedule="nope").create_state("cpu")


def test_param_store_layout_cpu():
    cfg = nets.unet_config("tiny")
    spec = nets.unet_spec(cfg)
    st = params.ParamStore(spec, device="cpu", quantise=True, quant_excluded=("bias", "scale", "conv_in", "conv_out", "time_embedding", "time_emb_proj"),
                           wd_excluded=("bias", "scale"), block_size=16, with_ema=True)
    w = nets.init_params(spec, 0)
    st.load(w)
    for k, v in w.items():
        assert torch.equal(st.p(k), v)
        lf = st.leaves[k]
        assert lf.quantised == (k.endswith("kernel") and not any(c in k.split("/") for c in ("conv_in", "conv_out", "time_embedding", "time_emb_proj")))
        assert lf.decayed == k.endswith("kernel")
    # segments are contiguous, block aligned, non-overlapping
    assert st.segments[0][2] == 0 and all(a[3] == b[2] for a, b in zip(st.segments, st.segments[1:])) and st.segments[-1][3] == st.total
    assert all(s[2] % 16 == 0 for s in st.segments)
    offs = sorted((lf.offset, lf.offset + lf.numel) for lf in st.leaves.values())
    assert all(a[1] <= b[0] for a, b in zip(offs, offs[1:]))
    assert torch.equal(st.ema, st.master)
    assert (st.codes == 3).all() and (st.inv_scale == 1).all()  # lion_quant.py:119-123
    ci = st.leaves["conv_in/kernel"]
    assert (ci.batch, ci.R, ci.C, ci.Rp, ci.Cp) == (9, 4, 32, 8, 32)
    ranges, owners = st.bucket_ranges(1 << 16)
    assert ranges[0][0] == 0 and ranges[-1][1] == st.total and all(owners)
    with pytest.raises(ValueError, match="quant_block_size"):
        params.ParamStore([("x/kernel", (3, 5))], device="cpu", quantise=True, block_size=16)


def test_context_assembly_matches_oracle():
    hs = torch.randn(6, 77, 16)
    for strip in (True, False):
        assert torch.equal(training_utils.assemble_context(hs, 2, strip), onets.assemble_context(hs, 2, strip))
        assert torch.equal(training_utils.assemble_context(hs[:2], 2, strip), onets.assemble_context(hs[:2], 2, strip))


def test_vae_decoder_spec_matches_oracle_tree():
    from oracle import nets as onets
    from stable_diffusion_training_amd import nets
    for name in ("sd", "tiny"):
        spec = dict(nets.vae_decoder_spec(nets.vae_config(name)))
        ref = onets.vae_decoder_param_shapes(onets.vae_config(name))
        assert {k: tuple(v) for k, v in spec.items()} == {k: tuple(v) for k, v in ref.items()}


def test_ddim_scheduler_tables_match_oracle():
    from oracle import schedulers as osched
    from stable_diffusion_training_amd.schedulers import DDIMScheduler
    for sched in ("scaled_linear", "zero_snr_scaled_linear"):
        d = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule=sched, prediction_type="v_prediction")
        st = osched.create_state(sched)
        assert np.array_equal(d.alphas_cumprod, st["alphas_cumprod"])
        for n in (20, 50):
            ts = d.set_timesteps(n)
            assert np.array_equal(ts, osched.ddim_timesteps(n))
            a_t, a_prev = d.alpha_products(ts[0])
            assert a_t == float(st["alphas_cumprod"][ts[0]]) and a_prev == float(st["alphas_cumprod"][ts[0] - 1000 // n])
            assert d.alpha_products(ts[-1])[1] == 1.0  # set_alpha_to_one past the last step
    with pytest.raises(ValueError):
        DDIMScheduler(prediction_type="nope")


def test_synthetic_streamer_ranks_walk_the_same_buckets():
    from stable_diffusion_training_amd.streamer import DataLoader
    from stable_diffusion_training_amd.training_utils import calculate_resolution_array
    kw = dict(training_batch_size=4, repeat_batch=3, maximum_resolution_areas=[256 ** 2], bucket_lower_bound_resolutions=[128],
              seed=7, context_concatenation_multiplier=3, batches_per_chunk=8, world_size=2)
    loaders = [DataLoader(rank=r, **kw) for r in range(2)]
    shapes = []
    for dl in loaders:
        dl._print_debug = False
        dl.create_training_dataframe()
        dl.dispatch_worker()
        assert dl._first_batch_count + dl._bulk_batch_count == 8
    buckets = {tuple(int(v) for v in b) for b in calculate_resolution_array(256 ** 2, 128, 64)}
    while True:
        b0, b1 = (dl.grab_next_batch() for dl in loaders)
        if b0 == "end_of_batch":
            assert b1 == "end_of_batch"
            break
        assert b0["pixel_values"].shape == b1["pixel_values"].shape and tuple(b0["pixel_values"].shape[:2]) == (2, 3)
        assert tuple(b0["pixel_values"].shape[2:]) in buckets
        assert not torch.equal(b0["pixel_values"], b1["pixel_values"])  # each rank its own shard
        assert tuple(b0["input_ids"].shape) == (2, 3 * 77) and b0["input_ids"].dtype == torch.int32
        assert int(b0["input_ids"].reshape(-1, 77)[:, 0].min()) == 49406 and int(b0["input_ids"].reshape(-1, 77)[:, -1].max()) == 49407
        shapes.append(tuple(b0["pixel_values"].shape))
    assert len(shapes) == 8 and shapes[0] == shapes[1] == shapes[2] and shapes[3] == shapes[4] == shapes[5]  # repeat_batch runs
    with pytest.raises(ValueError):
        DataLoader(training_batch_size=3, world_size=2)


def test_key_chunk_weights_match_oracle():
    for nq, nk in ((64, 77), (16, 77), (64, 227), (144, 231), (256, 77), (4096, 77), (77, 77)):
        ref = onets.key_chunk_weights(nq, nk)
        got = nets.key_chunk_weights(nq, nk, "cpu")
        assert (got is None and bool((ref == 1).all())) or torch.equal(got, ref), (nq, nk)


def test_sharded_store_refuses_export_until_gathered():
    """a save under `if rank == 0:` must not start a collective.  A store whose optimizer state is scattered raises on
    export until GradReducer.gather_state() (called on every rank) has made it whole."""
    st = params.ParamStore([("a/kernel", (8, 16)), ("a/bias", (16,))], device="cpu", quantise=True, quant_excluded=("bias",), with_ema=True)
    st.export()
    st.sharded, st.state_whole = True, False
    with pytest.raises(RuntimeError, match="gather_state"):
        st.export()
    with pytest.raises(RuntimeError, match="gather_state"):
        st.export_momentum()
    st.state_whole = True
    st.export("ema")


def test_gradient_leaf_single_use_per_step():
    """Dense / conv gradients are written, not accumulated: a leaf reported twice between zero_grad() and the optimizer step
    (tied weights, two encoder calls, micro-batches) is refused instead of silently keeping the last contribution."""
    from stable_diffusion_training_amd import ops
    st = params.ParamStore([("a/kernel", (8, 16)), ("a/bias", (16,))], device="cpu", quantise=False)
    ops._ready(st, "a/kernel")
    ops._ready(st, "a/kernel")  # not armed outside a step (kernel-level tests drive ops directly)
    st.zero_grad(everything=True)
    ops._ready(st, "a/kernel", "a/bias")
    with pytest.raises(RuntimeError, match="twice"):
        ops._ready(st, "a/kernel")
