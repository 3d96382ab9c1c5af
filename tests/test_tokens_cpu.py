"""New tokens (textual inversion) without a device: the numpy references (tests/token_reference.py) proven against
torch.nn.functional.embedding and its autograd over the resized table, TokenConfig / tokens.attach / state-builder / train_step
refusals, the token file, resized_tree, the streamer's placeholder option, and the library's three new exports with every host
refusal."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from oracle import nets as onets
from stable_diffusion_training_amd import _lib, lora, nets, tokens
from stable_diffusion_training_amd.params import ParamStore
from tests import token_reference as tr

TOK = "text_model/embeddings/token_embedding/embedding"
NEW = "text_model/embeddings/token_embedding/new_tokens"


def _clip_base(trainable=False, cfg=None, seed=3):
    cfg = cfg or onets.clip_config("tiny")
    st = ParamStore(nets.clip_text_spec(cfg), device="cpu", trainable=trainable, quantise=False)
    st.load(onets.init_params(onets.clip_param_shapes(cfg), seed))
    return st


# ------------------------------------------------------------------------------------------------ reference maths
@pytest.mark.parametrize("D", tr.SHAPES)
@pytest.mark.parametrize("n_ext", tr.N_EXT)
def test_references_are_embedding_and_its_autograd_over_the_resized_table(D, n_ext):
    """Integer-valued tables and gradients: every sum is exact in float32 whatever its order, so torch's embedding over the
    (V + n)-row table and its autograd's rows V... must equal the references bit for bit."""
    g = torch.Generator().manual_seed(D + n_ext)
    tok, ext, pos = (torch.randint(-8, 9, (r, D), generator=g).float() for r in (tr.V, n_ext, tr.S))
    for name, ids in tr.id_patterns(n_ext, 1).items():
        if name == "bad_ids":
            continue
        table = torch.cat([tok, ext]).requires_grad_(True)
        idl = torch.from_numpy(ids).long()
        out = torch.nn.functional.embedding(idl, table) + pos[torch.arange(ids.shape[0]) % tr.S]
        assert torch.equal(out.detach().to(torch.bfloat16), tr.forward_ref(ids, tok.numpy(), ext.numpy(), pos.numpy())), name
        dout = torch.randint(-3, 4, (ids.shape[0], D), generator=g).float()
        out.backward(dout)
        want = table.grad[tr.V:]
        got = tr.backward_ref(ids, dout.numpy(), tr.V, n_ext)
        assert np.array_equal(got, want.numpy()), name
        assert float(dout.abs().max()) * ids.shape[0] < 2 ** 24
    # ids outside both tables select a row of +0.0: pos alone
    ids = tr.id_patterns(n_ext, 1)["bad_ids"]
    out = tr.forward_ref(ids, tok.numpy(), ext.numpy(), pos.numpy())
    for r in tr.BAD_ROWS:
        assert torch.equal(out[r], pos[r % tr.S].to(torch.bfloat16))
    assert torch.equal(out[7], (ext[0] + pos[0]).to(torch.bfloat16))


def test_backward_reference_adds_in_row_order():
    ids = np.array([tr.V] * 4, np.int32)
    col = np.array([[2.0 ** 24], [1.0], [1.0], [-2.0 ** 24]], np.float32)
    assert tr.backward_ref(ids, col, tr.V, 1)[0, 0] == 0.0          # ((2^24 + 1) + 1) - 2^24 in float32: both ones are absorbed
    assert tr.backward_ref(ids, col[[1, 2, 0, 3]], tr.V, 1)[0, 0] == 2.0  # another order gives another sum
    assert all(torch.tensor(v).to(torch.bfloat16).item() == v for v in (2.0 ** 24, 1.0, -2.0 ** 24))


def test_retract_reference():
    g = np.random.default_rng(0)
    x = g.standard_normal((3, 12)).astype(np.float32) * 0.3
    mean, std = tr.retract_stats(x)
    assert abs(mean - x.astype(np.float64).mean()) < 1e-15 and abs(std - x.astype(np.float64).std(ddof=1)) < 1e-15
    f = tr.retract_factor(std, 0.02, 0.1)
    assert f.dtype == np.float32 and abs(float(f) - (0.02 / std) ** 0.1) < 1e-7
    assert tr.retract_factor(0.0, 0.02, 0.1) == 1.0
    assert tr.retract_stats(np.full((1, 8), 0.1, np.float32))[1] == 0.0


# ------------------------------------------------------------------------------------------------ TokenConfig / attach
def test_token_config_refusals():
    for kw, msg in ((dict(num_tokens=0), "num_tokens"), (dict(num_tokens=257), "num_tokens"), (dict(num_tokens=True), "num_tokens"),
                    (dict(num_tokens=2.0), "num_tokens"), (dict(num_tokens=2, init_ids=(1, 2, 3)), "init_ids"),
                    (dict(num_tokens=2, init_ids=(-1, 2)), "init_ids"), (dict(num_tokens=2, init_ids="ab"), "init_ids"),
                    (dict(num_tokens=2, seed=1.5), "seed"), (dict(num_tokens=2, retract=1), "retract"),
                    (dict(num_tokens=2, retract_power=float("nan")), "retract_power"), (dict(num_tokens=2, retract_power="x"), "retract_power")):
        with pytest.raises(ValueError, match=msg):
            tokens.TokenConfig(**kw)
    assert tokens.TokenConfig(3, init_ids=7).init_ids == (7, 7, 7)
    assert tokens.TokenConfig(2, init_ids=[4, 5]).init_ids == (4, 5)
    assert tokens.TokenConfig(256).init_ids is None


def test_attach_builds_the_token_store_and_initialises_it():
    base = _clip_base()
    V, D = base.leaves[TOK].shape
    ad = tokens.attach(base, tokens.TokenConfig(3, init_ids=(5, 0, V - 1)), with_ema=True)
    assert base.tokens is ad and base.adapter is None and ad.store.trainable and ad.store.order == [NEW]
    assert ad.store.leaves[NEW].shape == (3, D) and ad.store.grad16 is None and not ad.store.leaves[NEW].quantised
    assert ad.placeholder_ids() == [V, V + 1, V + 2] and ad.geometry == [(V, D)]
    assert torch.equal(ad.store.p(NEW), base.p(TOK)[[5, 0, V - 1]])  # bit for bit
    assert torch.equal(ad.store.ema, ad.store.master)
    assert ad.target_std == [float(base.p(TOK).double().std(unbiased=True))]
    assert ad.source == "master"
    ad.select("ema")
    assert ad.source == "ema" and ad.rows(TOK).data_ptr() == ad.store.ema.data_ptr() + 4 * ad.store.leaves[NEW].offset
    with pytest.raises(ValueError, match="source"):
        ad.select("best")
    # without init_ids: seeded normal rows at the base table's standard deviation
    a, b, c = (tokens.attach(_clip_base(), tokens.TokenConfig(64, seed=s)) for s in (1, 1, 2))
    assert torch.equal(a.store.master, b.store.master) and not torch.equal(a.store.master, c.store.master)
    assert abs(float(a.store.p(NEW).std()) / a.target_std[0] - 1) < 0.1
    with pytest.raises(ValueError, match="no EMA"):
        a.select("ema")
    # a quantising store keeps the new tokens out of the quantised segments
    q = tokens.attach(_clip_base(), tokens.TokenConfig(4), quantise=True, quant_excluded=("bias",))
    assert not q.store.leaves[NEW].quantised and q.store.quant_total == 0


def test_attach_on_two_towers_gives_one_leaf_per_tower():
    cfg = dict(towers=[onets.clip_config("tiny"), onets.clip_config("tiny")], prefixes=["text_encoder/", "text_encoder_2/"])
    base = ParamStore(nets.clip_text_spec(cfg), device="cpu", trainable=False, quantise=False)
    g = torch.Generator().manual_seed(0)
    base.load({p: torch.randn(base.leaves[p].shape, generator=g) for p in base.order})
    ad = tokens.attach(base, tokens.TokenConfig(2, init_ids=9))
    assert ad.store.order == ["text_encoder/" + NEW, "text_encoder_2/" + NEW]
    assert ad.prefixes == ["text_encoder/", "text_encoder_2/"] and len(ad.target_std) == 2
    for pre in ad.prefixes:
        assert torch.equal(ad.store.p(pre + NEW), base.p(pre + TOK)[[9, 9]])
    assert ad.placeholder_ids(1) == [base.leaves["text_encoder_2/" + TOK].shape[0] + j for j in range(2)]


def test_attach_refusals():
    cfg = tokens.TokenConfig(2)
    with pytest.raises(ValueError, match="frozen"):
        tokens.attach(_clip_base(trainable=True), cfg)
    base = _clip_base()
    tokens.attach(base, cfg)
    with pytest.raises(ValueError, match="already"):
        tokens.attach(base, cfg)
    with pytest.raises(ValueError, match="new tokens"):  # ... and no LoRA on a store that carries tokens
        lora.attach(base, lora.LoraConfig(rank=4, alpha=4, targets=lora.CLIP_TARGETS))
    adapted = _clip_base()
    lora.attach(adapted, lora.LoraConfig(rank=4, alpha=4, targets=lora.CLIP_TARGETS))
    with pytest.raises(ValueError, match="LoRA adapter"):
        tokens.attach(adapted, cfg)
    with pytest.raises(ValueError, match="TokenConfig"):
        tokens.attach(_clip_base(), dict(num_tokens=2))
    with pytest.raises(ValueError, match="vocabulary size"):
        tokens.attach(_clip_base(), tokens.TokenConfig(2, init_ids=onets.clip_config("tiny")["vocab_size"]))
    with pytest.raises(ValueError, match="no token table"):
        tokens.attach(ParamStore([("a/kernel", (8, 8))], device="cpu", trainable=False), cfg)
    with pytest.raises(ValueError, match="quant_mask"):
        tokens.attach(_clip_base(), cfg, quant_mask={NEW: True})


def test_state_builder_refusals():
    from stable_diffusion_training_amd import training_utils as tu
    cfg = tokens.TokenConfig(2)
    with pytest.raises(ValueError, match="new_tokens"):
        tu.create_lion_optimizer_states({}, new_tokens=dict(num_tokens=2), device="cpu")
    with pytest.raises(ValueError, match="new_tokens"):
        tu.create_lion_optimizer_states({}, new_tokens=cfg, train_unet=False, device="cpu")
    with pytest.raises(ValueError, match="new_tokens.*text-encoder LoRA"):
        tu.create_lion_optimizer_states({}, new_tokens=cfg, device="cpu",
                                        lora=dict(unet=lora.LoraConfig(4, 4), text_encoder=lora.LoraConfig(4, 4, targets=lora.CLIP_TARGETS)))


def test_state_builder_builds_frozen_bases_and_a_token_store():
    from stable_diffusion_training_amd import training_utils as tu
    ucfg, ccfg = onets.unet_config("tiny"), onets.clip_config("tiny")
    models = {"unet": {"unet_params": onets.init_params(onets.unet_param_shapes(ucfg), 1), "config": ucfg},
              "text_encoder": {"text_encoder_params": onets.init_params(onets.clip_param_shapes(ccfg), 3), "config": ccfg}}
    for lo in (None, dict(unet=lora.LoraConfig(4, 4), text_encoder="frozen")):
        out = tu.create_lion_optimizer_states(models, new_tokens=tokens.TokenConfig(2, init_ids=3), device="cpu", lora=lo,
                                              with_text_encoder_ema=True, text_encoder_learning_rate=7e-4)
        us, ts = out["unet_state"], out["text_encoder_state"]
        assert not us.store.trainable and not ts.store.trainable and ts.adapter is None
        assert ts.tokens is ts.store.tokens and ts.opt_store is ts.tokens.store and ts.tokens.store.ema is not None
        assert ts.hyper["lr"] == pytest.approx(7e-4 / 7) and ts.step == 0
        if lo is None:
            assert us.adapter is None and us.opt_store is None and us.hyper == {}
        else:
            assert us.opt_store is us.adapter.store and us.hyper


def test_train_step_refuses_a_reducer_and_mixed_states():
    from stable_diffusion_training_amd import training_utils as tu
    base = _clip_base()
    ad = tokens.attach(base, tokens.TokenConfig(2))
    ts = tu.TrainState(nets.clip_text_forward, base, onets.clip_config("tiny"), {}, None, ad)
    frozen_unet = tu.TrainState(None, ParamStore([("a/kernel", (8, 8))], device="cpu", trainable=False), {}, {})
    assert ts.opt_store is ad.store and frozen_unet.opt_store is None
    sched = tu.FrozenModel(call=None, params=None)
    with pytest.raises(ValueError, match="new tokens: data-parallel"):
        tu.train_step(frozen_unet, ts, None, None, {}, None, None, sched, reducer=object())
    trained_unet = tu.TrainState(None, ParamStore([("a/kernel", (8, 8))], device="cpu", trainable=False), {}, {})
    trained_unet.store.trainable = True
    with pytest.raises(ValueError, match="new tokens: mixed modes"):
        tu.train_step(trained_unet, ts, None, None, {}, None, None, sched)
    # the store carries tokens the state does not know of: its optimizer step would never run
    stray = tu.TrainState(nets.clip_text_forward, base, onets.clip_config("tiny"), {})
    with pytest.raises(ValueError, match="new tokens"):
        tu.train_step(frozen_unet, stray, None, None, {}, None, None, sched)


# ------------------------------------------------------------------------------------------------ token file, resized tree
def test_token_file_round_trip_and_mismatches(tmp_path):
    ad = tokens.attach(_clip_base(), tokens.TokenConfig(3, init_ids=(1, 2, 3)))
    g = torch.Generator().manual_seed(2)
    ad.store.master.copy_(torch.randn(ad.store.total, generator=g))
    path = str(tmp_path / "tokens.npz")
    ad.save(path)
    with np.load(path) as z:
        meta = __import__("json").loads(bytes(z["__meta__"]).decode())
        assert sorted(z.files) == ["__meta__", NEW]
    V, D = ad.geometry[0]
    assert meta == dict(num_tokens=3, towers=[dict(prefix="", vocab_size=V, width=D)], target_std=ad.target_std, init_ids=[1, 2, 3])
    fresh = tokens.attach(_clip_base(seed=4), tokens.TokenConfig(3, seed=9))
    fresh.load(path)
    assert torch.equal(fresh.store.p(NEW), ad.store.p(NEW)) and fresh.target_std == ad.target_std
    with pytest.raises(ValueError, match="3 tokens in the file, 2 attached"):
        tokens.attach(_clip_base(), tokens.TokenConfig(2)).load(path)
    wide = dict(onets.clip_config("tiny"), vocab_size=onets.clip_config("tiny")["vocab_size"] + 8)
    with pytest.raises(ValueError, match="another base geometry.*vocab_size"):
        tokens.attach(_clip_base(cfg=wide), tokens.TokenConfig(3)).load(path)
    np.savez(str(tmp_path / "plain.npz"), x=np.zeros(3))
    with pytest.raises(ValueError, match="not a token file"):
        ad.load(str(tmp_path / "plain.npz"))
    lo = lora.attach(_clip_base(), lora.LoraConfig(rank=4, alpha=4, targets=lora.CLIP_TARGETS))
    lo.save(str(tmp_path / "adapter.npz"))
    with pytest.raises(ValueError, match="not a token file"):
        ad.load(str(tmp_path / "adapter.npz"))


def test_resized_tree_and_config():
    from stable_diffusion_training_amd import checkpoint as ck
    base = _clip_base()
    ad = tokens.attach(base, tokens.TokenConfig(2, seed=5), with_ema=True)
    ad.store.ema.mul_(2.0)
    V, D = ad.geometry[0]
    for source in ("master", "ema"):
        tree = ad.resized_tree(source)
        assert set(tree) == set(base.order) and tree[TOK].shape == (V + 2, D)
        assert torch.equal(tree[TOK][:V], base.p(TOK)) and torch.equal(tree[TOK][V:], ad.rows(TOK, source))
        assert all(torch.equal(tree[p], base.p(p)) for p in base.order if p != TOK)
    assert not torch.equal(ad.resized_tree("master")[TOK], ad.resized_tree("ema")[TOK])
    cfg = onets.clip_config("tiny")
    assert ck._resized_text_config(cfg, ad) == dict(cfg, vocab_size=V + 2, num_new_tokens=2) and cfg["vocab_size"] == V
    assert ck._resized_text_config(ck._resized_text_config(cfg, ad), ad) == dict(cfg, vocab_size=V + 4, num_new_tokens=4)
    dual = dict(towers=[cfg, dict(cfg, vocab_size=V + 1)], prefixes=["text_encoder/", "text_encoder_2/"])
    assert [t["vocab_size"] for t in ck._resized_text_config(dual, ad)["towers"]] == [V + 2, V + 3]
    # what save_model serialises for the store and for the EMA view of the token store
    from stable_diffusion_training_amd.params import EmaView
    flat = ck.flatten_tree(ck.params_to_tree(base))
    assert flat[TOK].shape == (V + 2, D) and np.array_equal(flat[TOK][V:], ad.rows(TOK, "master").numpy())
    flat = ck.flatten_tree(ck.params_to_tree(EmaView(ad.store)))
    assert np.array_equal(flat[TOK][V:], ad.rows(TOK, "ema").numpy()) and ck._tokens_of(EmaView(ad.store)) is ad and ck._tokens_of(base) is ad
    # the resized tree loads into a plain store built from the resized config
    plain = ParamStore(nets.clip_text_spec(dict(cfg, vocab_size=V + 2)), device="cpu", trainable=False, quantise=False)
    plain.load(ad.resized_tree("master"))
    assert torch.equal(plain.p(TOK)[V:], ad.rows(TOK, "master"))


# ------------------------------------------------------------------------------------------------ streamer
def _digest(batch):
    h = hashlib.sha256()
    for k in sorted(batch):
        h.update(k.encode())
        h.update(batch[k].numpy().tobytes())
    return h.hexdigest()


def _loader(**kw):
    from stable_diffusion_training_amd.streamer import DataLoader
    dl = DataLoader(training_batch_size=2, maximum_resolution_areas=(64 ** 2,), bucket_lower_bound_resolutions=(64,), vocab_size=1000,
                    batches_per_chunk=2, **kw)
    dl._print_debug = False
    dl.create_training_dataframe()
    dl.dispatch_worker()
    return dl


def test_streamer_placeholder_ids():
    plain = _loader(context_concatenation_multiplier=2).grab_next_batch()
    assert _digest(plain) == _digest(_loader(context_concatenation_multiplier=2, placeholder_ids=None).grab_next_batch())
    got = _loader(context_concatenation_multiplier=2, placeholder_ids=[1000, 1001]).grab_next_batch()
    ids, ref = got["input_ids"].view(2, 2, 77), plain["input_ids"].view(2, 2, 77)
    assert bool((ids[..., 1:3] == torch.tensor([1000, 1001], dtype=torch.int32)).all())
    keep = torch.ones(77, dtype=torch.bool)
    keep[1:3] = False
    assert torch.equal(ids[..., keep], ref[..., keep]) and torch.equal(got["pixel_values"], plain["pixel_values"])
    assert bool((ids[..., 0] == 998).all()) and bool((ids[..., -1] == 999).all())
    # SDXL rows: ids per tower
    two = _loader(text_towers=2, placeholder_ids=[[1000], [2000]]).grab_next_batch()["input_ids"].view(2, 1, 2, 77)
    assert bool((two[:, :, 0, 1] == 1000).all()) and bool((two[:, :, 1, 1] == 2000).all())
    same = _loader(text_towers=2, placeholder_ids=[1000]).grab_next_batch()["input_ids"].view(2, 1, 2, 77)
    assert bool((same[:, :, :, 1] == 1000).all())
    for bad in ([], [[1], [2], [3]], [[1, 2], [3]], list(range(76))):
        with pytest.raises(ValueError, match="placeholder_ids"):
            _loader(text_towers=2, placeholder_ids=bad)


# ------------------------------------------------------------------------------------------------ exports
def test_library_exports_and_argument_checks(lib):
    assert lib.sdt_abi_version() == 5
    counts = {"sdt_embedding_ext_fwd": 11, "sdt_embedding_ext_bwd": 8, "sdt_embedding_retract": 7}
    for name, n in counts.items():
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name]) == n and len(getattr(lib, name).argtypes) == n
    p = 4096  # any aligned non-null address: every call below fails its checks before anything is launched
    INV = -1

    def fwd(ids=p, tok=p, ext=p, pos=p, out=p, rows=21, S=7, D=12, V=11, n=5):
        return lib.sdt_embedding_ext_fwd(ids, tok, ext, pos, out, rows, S, D, V, n, None)

    def bwd(ids=p, dout=p, dext=p, rows=21, D=12, V=11, n=5):
        return lib.sdt_embedding_ext_bwd(ids, dout, dext, rows, D, V, n, None)

    def retract(ext=p, n=5, D=12, target=0.02, power=0.1, stats=p):
        return lib.sdt_embedding_retract(ext, n, D, target, power, stats, None)

    for name in ("ids", "tok", "ext", "pos", "out"):
        assert fwd(**{name: None}) == INV and b"pointer" in lib.sdt_last_error(), name
        assert fwd(**{name: p + 1}) == INV and b"misaligned" in lib.sdt_last_error(), name
    for name in ("ids", "tok", "ext", "pos"):
        assert fwd(**{name: p + 2}) == INV, name  # float32 / int32 operands: 4-byte aligned
    for name in ("rows", "S", "D", "V"):
        for v in (0, -3):
            assert fwd(**{name: v}) == INV and b"positive" in lib.sdt_last_error(), (name, v)
    for v in (0, -1, 257):
        assert fwd(n=v) == INV and b"n_ext" in lib.sdt_last_error()
        assert bwd(n=v) == INV and b"n_ext" in lib.sdt_last_error()
        assert retract(n=v) == INV and b"n_ext" in lib.sdt_last_error()
    for name in ("ids", "dout", "dext"):
        assert bwd(**{name: None}) == INV and b"pointer" in lib.sdt_last_error(), name
        assert bwd(**{name: p + 1}) == INV, name
    assert bwd(ids=p + 2) == INV and bwd(dext=p + 2) == INV
    for name in ("rows", "D", "V"):
        for v in (0, -3):
            assert bwd(**{name: v}) == INV and b"positive" in lib.sdt_last_error(), (name, v)
    for name in ("ext", "stats"):
        assert retract(**{name: None}) == INV and b"pointer" in lib.sdt_last_error(), name
    assert retract(ext=p + 2) == INV and retract(stats=p + 4) == INV
    assert retract(D=0) == INV and retract(D=-1) == INV
    for v in (0.0, -1.0, float("inf"), float("nan")):
        assert retract(target=v) == INV and b"target_std" in lib.sdt_last_error(), v
    for v in (float("inf"), float("nan")):
        assert retract(power=v) == INV, v
    assert ctypes.sizeof(ctypes.c_double) == 8
