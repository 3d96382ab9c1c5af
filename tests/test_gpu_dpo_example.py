"""examples/train_synthetic.py with `dpo_beta` set beside `lora_rank` (its --lora RANK --dpo BETA switches) on the golden config, tiny
model: the loader emits pairs, the captured DPO steps run, the log carries implicit_acc, the adapter trains and its file is written;
without `lora_rank` the configuration is refused."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests.helpers import make_case

pytestmark = pytest.mark.gpu


def test_training_loop_with_dpo_logs_the_accuracy_and_trains_the_adapter(tmp_path):
    from oracle import nets as onets
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(root, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    case = make_case("tiny", B=2, image=64)
    vae_w = dict(case["weights"]["vae"])
    vae_w.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), 9))
    models = {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
              "vae": {"vae_params": vae_w, "config": case["cfgs"]["vae"]},
              "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}, "tokenizer": None}
    cfg = json.load(open(os.path.join(root, "tests", "golden", "model_properties_keys.json")))
    cfg.pop("_note")
    cfg.update(model_path=str(tmp_path / "model@0"), batch_size=4, image_area_root=[64], minimum_axis_length=[64],
               context_window_concatenation_count=1, strip_bos_eos_token=False, beta_scheduler="scaled_linear", prediction_type="epsilon",
               ema_rate=0.99, repeat_batch=3, chunk_number=0, chunk_steps=1, chunk_limit=1, keep_trained_model_buffer=1, master_seed=3,
               loss_logging_interval=2, loss_csv=str(tmp_path / "loss.csv"), test_save_path=str(tmp_path / "test_save"),
               batches_per_chunk=5, DEBUG=False, dpo_beta=5000.0)
    with pytest.raises(ValueError, match="needs a LoRA / DoRA adapter"):
        mod.main(dict(cfg), models=models, log=lambda *_: None)
    lines = []
    losses, us, ts = mod.main(dict(cfg, lora_rank=8), models=models, log=lines.append)
    ad = us.adapter
    assert ad is not None and ts.adapter is None and all(np.isfinite(losses)) and len(losses) >= 2
    assert losses[0] == float(np.float32(np.log(2.0))), "the first step of a fresh adapter sits on the reference: loss ln 2"
    assert lines and all("implicit_acc" in ln for ln in lines), lines
    assert float(ad.store.p(ad.adapted[ad.paths[0]][1]).abs().max()) > 0, "B never left zero: the adapter did not train"
    assert os.path.isfile(tmp_path / "model-lora.npz")
