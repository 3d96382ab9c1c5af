"""examples/train_synthetic.py with `lora_rank` set (its --lora switch) on the golden config, tiny model: the loop runs, and what it
leaves behind is complete - the checkpoint with the adapter folded in, its -EMA twin folded from the adapter's EMA, the training-state
file and the adapter file - although the frozen text encoder has no EMA view (the golden config accumulates both EMAs)."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

from tests.helpers import make_case

pytestmark = pytest.mark.gpu


def test_training_loop_with_lora_saves_folded_checkpoints_state_and_adapter(tmp_path):
    from oracle import nets as onets
    from stable_diffusion_training_amd import lora
    from stable_diffusion_training_amd import training_utils as tu
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
    assert cfg["accumulate_unet_ema"] and cfg["accumulate_text_encoder_ema"]  # the frozen tower still has no EMA view
    cfg.update(model_path=str(tmp_path / "model@0"), batch_size=2, image_area_root=[128], minimum_axis_length=[64],
               context_window_concatenation_count=1, strip_bos_eos_token=False, beta_scheduler="scaled_linear", prediction_type="epsilon",
               ema_rate=0.99, repeat_batch=3, chunk_number=0, chunk_steps=1, chunk_limit=1, keep_trained_model_buffer=1, master_seed=3,
               loss_logging_interval=2, loss_csv=str(tmp_path / "loss.csv"), test_save_path=str(tmp_path / "test_save"),
               batches_per_chunk=5, DEBUG=False, lora_rank=8)
    losses, us, ts = mod.main(cfg, models=models, log=lambda *_: None)
    ad = us.adapter
    assert ad is not None and ad.cfg.rank == 8 and ts.adapter is None and not us.store.trainable and not ts.store.trainable
    assert us.step > 0 and us.store.count == 0 and all(np.isfinite(losses))
    assert os.path.isdir(tmp_path / "model@1") and os.path.isdir(tmp_path / "model-EMA@1")
    assert os.path.isfile(tmp_path / "model-state.safetensors") and os.path.isfile(tmp_path / "model-lora.npz")
    # the checkpoints are ordinary ones with the adapter folded in: from the masters, and from the adapter's EMA
    p = ad.paths[0]
    q = "conv_in/kernel"
    for d, source in (("model@1", "master"), ("model-EMA@1", "ema")):
        loaded = tu.load_models(types.SimpleNamespace(model_path=str(tmp_path / d)))
        want = ad.folded(source=source)
        assert torch.equal(loaded["unet"]["unet_params"][p].to("cuda:0"), want[p]), (d, p)
        assert torch.equal(loaded["unet"]["unet_params"][q].to("cuda:0"), us.store.p(q)), (d, q)
        k = next(iter(ts.store.leaves))
        assert torch.equal(loaded["text_encoder"]["text_encoder_params"][k].to("cuda:0"), ts.store.p(k))
    assert float(ad.store.p(ad.adapted[p][1]).abs().max()) > 0, "B never left zero: the adapter did not train"
    assert not torch.equal(ad.store.master, ad.store.ema)
    # the adapter file holds the trained factors
    fresh = tu.ParamStore([(n, us.store.leaves[n].shape) for n in us.store.order], device="cuda:0", trainable=False)
    fresh.load(case["weights"]["unet"])
    other = lora.attach(fresh, lora.LoraConfig(8, 8.0, seed=99))
    other.load(str(tmp_path / "model-lora.npz"))
    for n in ad.store.order:  # (leaf by leaf: the alignment gaps of a master buffer belong to no leaf and are in no file)
        assert torch.equal(other.store.p(n), ad.store.p(n)), n
