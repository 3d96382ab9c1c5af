"""CPU-side checks of micro-batch gradient accumulation: argument validation of sdt_grad_accumulate (it returns before any HIP
call, so no device is needed) and the host-side refusals of train_step / the step table."""
import ctypes

import pytest

ACC_INIT, ACC_ADD, ACC_FINISH, ACC_SCALE = 0, 1, 2, 3


def _aligned(buf, off=0):
    """An address inside `buf` that is 16-byte aligned, plus `off` bytes."""
    a = ctypes.addressof(buf)
    return (a + 15) // 16 * 16 + off


def test_grad_accumulate_argument_validation(lib):
    buf = ctypes.create_string_buffer(1 << 12)
    acc, g = _aligned(buf), _aligned(buf, 2048)
    f = lib.sdt_grad_accumulate
    # null accumulator, null gradient outside the scale mode
    assert f(None, g, 0, 16, ACC_ADD, 1.0, None, None, 0, None) == -1
    assert b"null pointer" in lib.sdt_last_error()
    assert f(acc, None, 0, 16, ACC_INIT, 1.0, None, None, 0, None) == -1
    assert b"null pointer" in lib.sdt_last_error()
    assert f(acc, g, 0, -4, ACC_ADD, 1.0, None, None, 0, None) == -1
    assert b"negative n" in lib.sdt_last_error()
    # alignment: acc 16 B; g 16 B as fp32, 8 B as bf16
    assert f(acc + 8, g, 0, 16, ACC_ADD, 1.0, None, None, 0, None) == -1
    assert b"acc must be 16-byte aligned" in lib.sdt_last_error()
    assert f(acc, g + 8, 0, 16, ACC_ADD, 1.0, None, None, 0, None) == -1
    assert b"g must be 16-byte aligned" in lib.sdt_last_error()
    assert f(acc, g + 4, 1, 16, ACC_ADD, 1.0, None, None, 0, None) == -1
    assert b"g must be 8-byte aligned" in lib.sdt_last_error()
    # unknown mode
    for bad in (-1, 4, 99):
        assert f(acc, g, 0, 16, bad, 1.0, None, None, 0, None) == -1
        assert b"unknown mode" in lib.sdt_last_error()
    # a norm needs the reduction workspace
    sq = _aligned(buf, 1024)
    assert f(acc, g, 0, 16, ACC_FINISH, 0.5, sq, None, 0, None) == -1
    assert b"workspace" in lib.sdt_last_error()
    assert f(acc, g, 0, 16, ACC_FINISH, 0.5, sq, _aligned(buf, 512), 64, None) == -1
    assert b"workspace" in lib.sdt_last_error()


def test_grad_accumulate_is_bound_and_the_abi_is_unchanged(lib):
    from stable_diffusion_training_amd import _lib
    assert "sdt_grad_accumulate" in _lib.SIGNATURES
    assert lib.sdt_abi_version() == 5


def test_param_store_accumulate_modes():
    from stable_diffusion_training_amd.params import ParamStore
    assert ParamStore.ACC_MODES == {"init": ACC_INIT, "add": ACC_ADD, "finish": ACC_FINISH, "scale": ACC_SCALE}


def test_step_table_keys_are_the_loader_batch_with_micro_batches():
    import torch

    from stable_diffusion_training_amd import training_utils as tu
    from tests.helpers import make_case

    case = make_case("tiny", B=2, image=64)

    class _S:  # the table builder reads only the store's device
        store = type("st", (), {"device": torch.device("cpu")})()

    tc = tu.TrainingConfig(
        model_path="synthetic", batch_size=2, learning_rate=1e-6, unet_learning_rate=1e-6, text_encoder_learning_rate=1e-6,
        lr_scheduler="constant", adam_to_lion_scale_factor=7.0, compilation_cache_path="", keep_compiled_fn_in_cache=False,
        text_encoder_context_window=77, context_window_concatenation_count=1, aot_compile=True, strip_bos_eos_token=False,
        offset_noise_magnitude=0.0, min_snr_gamma_magnitude=0.0, perturbation_noise_magnitude=0.0, image_area_root=[512],
        minimum_axis_length=[512], beta_scheduler=case["sched"], prediction_type="epsilon",
        excluded_layer_pattern_from_weight_decay=[], excluded_layer_from_quantization=[], quant_block_size=16,
        quantize_unet_state=True, quantize_text_encoder_state=True, accumulate_unet_ema=False, accumulate_text_encoder_ema=False,
        ema_rate=0.0)
    table = tu.dp_compile_all_unique_resolution(_S(), _S(), None, None, None, None, tc, per_device_batch=2, use_graph=False,
                                                micro_batches=4)
    assert list(table) == [(8, 3, 512, 512)]
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="micro_batches"):
            tu.dp_compile_all_unique_resolution(_S(), _S(), None, None, None, None, tc, use_graph=False, micro_batches=bad)
