"""Training Regulation + head on a frozen trunk (cf_trunk_outputs, cf_forward_train_x0, cf_x0_gather*, cf_reduce_opt_x0;
Trainer(freeze_trunk=True), TrunkCache, the requires_grad_(False) drop-in path, train --init-from / --freeze-trunk).

Referee: the CPU oracle with its Embedding / Pairwise parameters frozen and torch.optim.AdamW over the rest.  Bounds are taken from the
files that already bound the same quantities: LOGIT_TOL of tests/test_config_variants_gpu.py for activations, the margins of
tests/test_gpu_parity.py::test_three_adamw_steps_track_oracle for a short optimisation run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

from oracle import chromoformer_oracle as orc
from tests import unstructured_inputs as ui
from tests.helpers import build_model, perturbed_params
from tests.synth_data import make_dataset
from tests.test_config_variants_gpu import LOGIT_TOL, VARIANTS
from tests.test_embed_dense_gpu import CFG2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
CONFIGS = {"default": None, "embed_2_layers": CFG2}
CONFIGS.update({k: VARIANTS[k] for k in ("i_max4", "i_max16_unfused", "four_heads", "reg_4_heads", "odd_lengths", "d_emb_64", "d_emb_256")})


def _is_trunk(k):
    return k.startswith(("embed.", "pairwise_interaction."))


def _state(model):
    torch.cuda.synchronize()
    return {"params": model._flat.cpu().clone(), "m": model._mflat.cpu().clone(), "v": model._vflat.cpu().clone()}


def _split(model):
    from chromoformer_amd import _lib
    off, n = C.c_longlong(), C.c_longlong()
    _lib.check(_lib.lib().cf_grad_bucket(model._handle, _lib.BUCKET_REG, C.byref(off), C.byref(n)), "cf_grad_bucket")
    return off.value, off.value + n.value


# ----------------------------------------------------------------------------- 1. trunk outputs
@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("kind", ["realistic", "unstructured"])
def test_trunk_outputs_match_the_oracle_and_the_forward(name, kind):
    cfg = orc._cfg(CONFIGS[name])
    B = 5
    batch = orc.synthetic_batch(B, cfg=cfg, seed=13, regime="realistic") if kind == "realistic" else ui.unstructured_batch(B, cfg)
    P = perturbed_params(False, cfg)
    model = build_model(cfg, False, B)
    model.load_state_dict(P)
    with torch.no_grad():
        _, stages = orc.forward(P, batch, cfg, return_stages=True)
    got = model.trunk_outputs(*[batch[k] for k in ARGS])
    torch.cuda.synchronize()
    assert list(got) == list(cfg["binsizes"])
    for b in cfg["binsizes"]:
        ref = torch.cat([stages["embed_tss.%d" % b], stages["pairwise.%d" % b]], dim=1)
        assert got[b].shape == ref.shape == (B, cfg["i_max"] + 1, cfg["d_emb"])
        err = (got[b].cpu() - ref).abs().max().item()
        print("%s %s binsize %d: max |trunk_outputs - oracle| = %.3e" % (name, kind, b, err))
        assert err < LOGIT_TOL, (name, b, err)
    with torch.no_grad():
        model(*[batch[k] for k in ARGS])
    for r, b in enumerate(cfg["binsizes"]):
        buf = model.debug_buffer("R%d.x0" % r)[: got[b].numel()].view_as(got[b])
        assert torch.equal(buf, got[b]), (name, b)
    # a packed batch gives the same bits
    again = model.trunk_outputs(model.pack_batch(batch))
    assert all(torch.equal(again[b], got[b]) for b in got)


# ----------------------------------------------------------------------------- 2. frozen means untouched / 3. same arithmetic for the top
@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("use_graph", [False, True])
def test_frozen_steps_leave_the_trunk_untouched(reg, use_graph):
    from chromoformer_amd.engine import Trainer
    B = 6
    model = build_model(None, reg, B)
    model.load_state_dict(perturbed_params(reg))
    batches = [orc.synthetic_batch(B, seed=21 + i, regime="realistic", regression=reg) for i in range(2)]
    tr = Trainer(model, lr=1e-3, freeze_trunk=True, use_graph=use_graph)
    assert tr.rider_tiles == 0 and not tr.fuse_opt
    slots = [tr.stage(b) for b in batches]
    tr.step(slots[0])                                   # (the first pass builds the tiled copies)
    before = _state(model)
    x0_before = {b: t.clone() for b, t in model.trunk_outputs(slots[0]).items()}
    torch.cuda.synchronize()
    for i in range(4):
        tr.step(slots[i % 2])
    after = _state(model)
    lo, hi = _split(model)
    for k in before:
        assert torch.equal(before[k][:lo], after[k][:lo]), k                        # Embedding + Pairwise: parameters and both moments
        assert torch.equal(before[k][hi:], after[k][hi:]), k                        # the never-trained tail
    assert not torch.equal(before["params"][lo:hi], after["params"][lo:hi])
    assert float(after["m"][:lo].abs().max()) == 0.0 and float(after["v"][:lo].abs().max()) == 0.0
    # the tiled copies the trunk kernels read: the trunk computes the same bits as before the steps
    x0_after = model.trunk_outputs(slots[0])
    assert all(torch.equal(x0_before[b], x0_after[b]) for b in x0_before)
    named = dict(model.named_parameters())
    assert all(p.grad is None for k, p in named.items() if _is_trunk(k))


@pytest.mark.parametrize("reg", [False, True])
def test_top_gradients_and_first_step_equal_the_unfrozen_step(reg):
    from chromoformer_amd.engine import Trainer
    B = 6
    batch = orc.synthetic_batch(B, seed=33, regime="realistic", regression=reg)
    P = perturbed_params(reg)

    def run(**kw):
        model = build_model(None, reg, B)
        model.load_state_dict(P)
        tr = Trainer(model, lr=1e-3, keep_grads=True, use_graph=False, **kw)
        logits, loss = tr.step(tr.stage(batch))
        torch.cuda.synchronize()
        return model, logits.cpu().clone(), loss.cpu().clone(), model._gflat.cpu().clone(), _state(model)

    m0, lg0, ls0, g0, s0 = run(fuse_opt=False, merge_opt=False)
    m1, lg1, ls1, g1, s1 = run(freeze_trunk=True)
    lo, hi = _split(m1)
    assert torch.equal(lg0, lg1) and torch.equal(ls0, ls1)
    assert torch.equal(g0[lo:hi], g1[lo:hi])
    assert m1.active_grads().data_ptr() == m1._gflat[lo:].data_ptr() and m1.active_grads().numel() == hi - lo
    for k in s0:
        assert torch.equal(s0[k][lo:hi], s1[k][lo:hi]), k
    assert float(g1[:lo].abs().max()) == 0.0              # the trunk's range of the gradient buffer was never written
    # a full backward afterwards writes every gradient: active_grads() is the whole trainable range again
    m1.forward_backward(m1.pack_batch(batch), batch["label"])
    assert m1.active_grads().numel() == m1._layout.n_active and m1.active_grads().data_ptr() == m1._gflat.data_ptr()


# ----------------------------------------------------------------------------- 4. cache equals recompute
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("name,reg", [("default", False), ("default", True), ("d_emb_64", False), ("d_emb_256", False), ("embed_2_layers", False),
                                      ("reg_4_heads", False), ("i_max4", True)])
def test_cached_steps_equal_recomputed_steps(name, reg, use_graph):
    from chromoformer_amd.engine import EpochFeed, Trainer, TrunkCache
    from chromoformer_amd.synth import synthetic_store
    cfg = orc._cfg(CONFIGS[name])
    B, n, K = 4, 22, 7
    store = synthetic_store(n, torch.device("cuda", 0), seed=5, regime="realistic", regression=reg, n_feats=cfg["n_feats"], i_max=cfg["i_max"],
                            binsizes=tuple(cfg["binsizes"]), w_max=cfg["w_max"])
    P = perturbed_params(reg, cfg)
    g = torch.Generator().manual_seed(1)
    epochs = [torch.randperm(n, generator=g)[: (n // B) * B].view(-1, B).tolist() for _ in range(2)]

    def run(cached):
        model = build_model(cfg, reg, B)
        model.load_state_dict(P)
        tr = Trainer(model, lr=1e-3, freeze_trunk=True, use_graph=use_graph)
        cache = TrunkCache(model, store, 3) if cached else None       # (built in batches that do not divide the store: the tail batch)
        feed = EpochFeed(model, store, B, cache=cache)
        trace, k = [], 0
        for batches in epochs:
            feed.begin_epoch(batches, tr.stream)
            for _ in batches:
                if k == K:
                    break
                logits, loss = tr.step(feed.slot)
                with torch.cuda.stream(tr.stream):
                    trace.append((logits.clone(), loss.clone(), model._flat.clone(), model._mflat.clone(), model._vflat.clone()))
                k += 1
            assert feed.check(tr.stream) == 0
        torch.cuda.synchronize()
        return trace, feed.window(0, K - len(epochs[0]))      # (the step log of the second epoch's steps)

    a, wa = run(False)
    b, wb = run(True)
    assert len(a) == len(b) == K
    for s, (x, y) in enumerate(zip(a, b)):
        for what, u, v in zip(("logits", "loss", "params", "exp_avg", "exp_avg_sq"), x, y):
            assert torch.equal(u, v), (name, s, what, (u - v).abs().max().item())
    for u, v in zip(wa, wb):                               # the step logs (logits / labels / losses of the last epoch's steps)
        assert torch.equal(u, v)
    assert not torch.equal(a[0][2], a[-1][2])


# ----------------------------------------------------------------------------- 5. against the referee
@pytest.mark.parametrize("reg", [False, True])
def test_frozen_training_run_matches_oracle_adamw_with_a_frozen_trunk(tmp_path, reg, monkeypatch):
    """The run of tests/test_train_gpu.py::test_training_run_matches_reference_checkpoint -- the synthetic dataset of 48 genes, bsz 8,
    2 epochs x 4 steps, lr 3e-5 with StepLR -- with --freeze-trunk, against the CPU oracle on the same batches with its Embedding /
    Pairwise parameters frozen and torch.optim.AdamW + StepLR over the rest.  Margins: exactly that test's (validation scores 1e-3
    classifier / 5e-3 regressor, validation loss 2e-3 relative, squared-sum parameter checksums 1e-4 of the largest)."""
    import pandas as pd
    from chromoformer_amd import train
    from chromoformer_amd.data import ChromoformerDataset, shard_indices
    from tests.helpers import checksum
    npy = str(tmp_path / "npy")
    meta_path = make_dataset(npy, n_genes=48, seed=2024)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "chromoformer_amd", "configs", "default.yaml")))
    cfg["bsz"], cfg["num_epoch"] = 8, 3
    cfg_path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    perms = []
    draw = train.epoch_permutation
    monkeypatch.setattr(train, "epoch_permutation", lambda n: perms.append(draw(n)) or perms[-1])      # (the run's own shuffles, observed)
    out = str(tmp_path / "ck.pt")
    argv = ["-o", out, "-c", cfg_path, "--exp-id", "fz5", "-m", meta_path, "-d", npy, "--fold", "0", "--binsizes", "2000", "500", "100", "--freeze-trunk"]
    assert train.main(argv + (["--regression"] if reg else [])) == 0
    c = torch.load(out, map_location="cpu", weights_only=False)
    assert len(perms) == 2 and c["epoch"] == 2

    # the referee: the same splits (train.py:280-287), the same batches, the oracle's arithmetic
    meta = pd.read_csv(meta_path).sample(frac=1, random_state=cfg["seed"]).reset_index(drop=True)
    qs = [meta[meta.split == k].gene_id.tolist() for k in (1, 2, 3, 4)]
    train_genes, val_genes = qs[0] + qs[1] + qs[2], qs[3]
    mk = lambda genes: ChromoformerDataset(meta_path, npy, genes, cfg["n_feats"], cfg["i_max"], [2000, 500, 100], cfg["w_prom"], cfg["w_max"], regression=reg)
    ds, dv = mk(train_genes), mk(val_genes)
    collate = lambda d, idx: torch.utils.data.default_collate([d[i] for i in idx])
    P = orc.init_params(None, 42, reg)
    for k, t in P.items():
        t.requires_grad_(not _is_trunk(k) and not orc.never_trained(k))
    trunk0 = {k: v.detach().clone() for k, v in P.items() if _is_trunk(k)}
    opt = torch.optim.AdamW([t for t in P.values() if t.requires_grad], lr=float(cfg["lr"]))
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=cfg["gamma"])
    for perm in perms:
        for idx in shard_indices(perm, 0, 1, 8, drop_last=True):
            batch = collate(ds, idx)
            opt.zero_grad()
            orc.loss_fn(orc.forward(P, batch), batch["label"], reg).backward()
            opt.step()
        sched.step()
    with torch.no_grad():
        vb = collate(dv, range(len(dv)))
        ref_loss, ref_score, _ = train.validation_metrics(orc.forward(P, vb).numpy(), vb["label"].numpy(), reg)
    d_score = np.abs(np.asarray(c["val_score"]) - np.asarray(ref_score)).max()
    d_loss = abs(float(c["last_val_loss"]) - float(ref_loss))
    got = np.array([checksum(v) for v in c["net"].values()])
    ref = np.array([checksum(P[k]) for k in c["net"]])
    d_sum = np.abs(got[:, 2] - ref[:, 2]).max()
    print("frozen run vs oracle + AdamW (%s): val_score %.3e, val_loss %.3e (of %.4f), checksum %.3e (bound %.3e)" % (
        "regressor" if reg else "classifier", d_score, d_loss, float(ref_loss), d_sum, 1e-4 * ref[:, 2].max()))
    assert np.allclose(np.asarray(c["val_label"], dtype=np.float64), vb["label"].numpy().astype(np.float64), atol=1e-6)
    assert d_score < (5e-3 if reg else 1e-3)
    assert d_loss < 2e-3 * max(1.0, float(ref_loss))
    assert d_sum <= 1e-4 * ref[:, 2].max()
    assert all(torch.equal(c["net"][k], v) for k, v in trunk0.items())      # both sides: the trunk is where it started


# ----------------------------------------------------------------------------- 6. drop-in
def test_drop_in_freeze_matches_the_oracle():
    B = 4
    model = build_model(None, False, B)
    P = orc.init_params(None, 42, False)
    model.freeze_trunk()
    for k, t in P.items():
        t.requires_grad_(not _is_trunk(k) and not orc.never_trained(k))
    opt_ref = torch.optim.AdamW([t for t in P.values() if t.requires_grad], lr=1e-3)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    trunk0 = {k: p.detach().cpu().clone() for k, p in model.named_parameters() if _is_trunk(k)}
    for s in range(3):
        batch = orc.synthetic_batch(B, seed=100 + s, regime="realistic")
        opt_ref.zero_grad()
        ref_loss = orc.loss_fn(orc.forward(P, batch), batch["label"], False)
        ref_loss.backward()
        opt_ref.step()
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(*[batch[k] for k in ARGS]), batch["label"].long().cuda())
        loss.backward()
        named = dict(model.named_parameters())
        assert all(p.grad is None for k, p in named.items() if _is_trunk(k))
        assert all(p.grad is not None for k, p in named.items() if not _is_trunk(k) and not orc.never_trained(k))
        opt.step()
        assert abs(loss.item() - ref_loss.item()) < 2e-4                  # (the margins of test_three_adamw_steps_track_oracle)
    sd = model.state_dict()
    worst = max((sd[k].cpu() - P[k].detach()).abs().max().item() for k in P)
    assert worst < 2e-4, worst
    assert all(torch.equal(sd[k].cpu(), v) for k, v in trunk0.items())


def test_drop_in_mixed_freeze_raises_and_unfrozen_is_unchanged():
    from chromoformer_amd import _lib
    B = 4
    batch = orc.synthetic_batch(B, seed=7, regime="realistic")
    model = build_model(None, False, B)
    model.load_state_dict(perturbed_params())
    args = [batch[k] for k in ARGS]
    name = "pairwise_interaction.500.transformer.layers.1.ff.l1.weight"
    dict(model.named_parameters())[name].requires_grad_(False)
    with pytest.raises(RuntimeError) as e:
        model(*args).sum().backward()
    assert "embed.2000.lin_proj.weight" in str(e.value) and name in str(e.value) and "whole trunk" in str(e.value)
    model.freeze_trunk(False)
    top = "regulation.2000.transformer.layers.0.ff.l1.bias"
    dict(model.named_parameters())[top].requires_grad_(False)
    with pytest.raises(RuntimeError) as e:
        model(*args).sum().backward()
    assert top in str(e.value) and "whole trunk" in str(e.value)
    dict(model.named_parameters())[top].requires_grad_(True)
    # nothing frozen: the gradients of cf_backward_from called directly, bit for bit
    out = model(*args)
    dl = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).cuda()
    out.backward(dl)
    torch.cuda.synchronize()
    g_hook = model._gflat.cpu().clone()
    model._gflat.zero_()
    bs, keep = model.pack_batch(batch)
    model._run_forward(bs, save=True)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().cf_backward_from(model._handle, C.byref(bs), dl.data_ptr(), st), "cf_backward_from")
    torch.cuda.synchronize()
    assert torch.equal(g_hook, model._gflat.cpu())
    assert all(p.grad is not None for k, p in model.named_parameters() if not orc.never_trained(k))


# ----------------------------------------------------------------------------- 7. guards
def test_guards():
    from chromoformer_amd import _lib
    from chromoformer_amd.engine import EpochFeed, Trainer, TrunkCache
    from chromoformer_amd.synth import synthetic_store
    B = 4
    model = build_model(None, False, B)
    with pytest.raises(ValueError, match="freeze_trunk=True is not supported with data parallelism"):
        Trainer(model, freeze_trunk=True, world_size=2)
    store = synthetic_store(8, torch.device("cuda", 0), seed=5, regime="realistic")
    tr = Trainer(model, lr=1e-3, freeze_trunk=True, use_graph=False)
    cache = TrunkCache(model, store)
    feed = EpochFeed(model, store, B, cache=cache)
    feed.begin_epoch([[0, 1, 2, 3], [4, 5, 6, 7]], tr.stream)
    tr.step(feed.slot)
    # part 4 after the x0 forward: refused by name
    L, st = _lib.lib(), tr.stream.cuda_stream
    rc = L.cf_backward_part(model._handle, C.byref(feed.slot.struct), feed.slot.label.data_ptr(), 1.0, feed.slot.loss.data_ptr(), 4, st)
    assert rc != 0 and "cf_forward_train_x0" in L.cf_last_error().decode() and "parts & 4" in L.cf_last_error().decode()
    # a trunk parameter written through torch: the cache refuses the next step, by name
    with torch.no_grad():
        dict(model.named_parameters())["embed.500.lin_proj.weight"].mul_(1.5)
    with pytest.raises(RuntimeError, match=r"TrunkCache is stale.*rebuild\(\).*params_changed\(\)"):
        tr.step(feed.slot)
    cache.rebuild()
    tr.step(feed.slot)
    assert feed.check(tr.stream) == 0
    # a Regulation parameter written through torch does not stale the cache
    with torch.no_grad():
        dict(model.named_parameters())["fc_head.2.bias"].add_(0.5)
    cache.check()
    # a pending backward() across trunk_outputs() behaves as across attention_maps()
    torch.cuda.synchronize()
    batch = orc.synthetic_batch(B, seed=7, regime="realistic")
    out = model(*[batch[k] for k in ARGS])
    model.trunk_outputs(*[batch[k] for k in ARGS])
    with pytest.raises(RuntimeError, match="trunk_outputs"):
        out.sum().backward()


# ----------------------------------------------------------------------------- 8. entry point
@pytest.mark.parametrize("reg", [False, True])
def test_train_entry_point_warm_start_on_a_frozen_trunk(tmp_path, reg, capsys):
    from chromoformer_amd import ChromoformerClassifier, ChromoformerRegressor, train
    from chromoformer_amd.net import split_layout
    meta = make_dataset(str(tmp_path / "npy"), n_genes=48, seed=2024)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "chromoformer_amd", "configs", "default.yaml")))
    cfg["bsz"], cfg["num_epoch"] = 8, 3
    cfg_path = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    Model = ChromoformerRegressor if reg else ChromoformerClassifier
    src = Model(seed=7)
    ck = str(tmp_path / "init.pt")
    torch.save({"net": src.state_dict(), "optimizer": {"state": {0: "not taken"}}, "epoch": 9}, ck)
    out = str(tmp_path / "ck.pt")
    argv = ["-o", out, "-c", cfg_path, "--exp-id", "fz", "-m", meta, "-d", str(tmp_path / "npy"), "--fold", "0", "--binsizes", "2000", "500", "100",
            "--init-from", ck, "--freeze-trunk", "--timing"] + (["--regression"] if reg else [])
    assert train.main(argv) == 0
    assert "trunk cache build" in capsys.readouterr().out
    c = torch.load(out, map_location="cpu", weights_only=False)
    init = src.state_dict()
    assert list(c["net"]) == list(init) and os.path.exists(out + ".done")
    trunk, top, never = split_layout(src._table)
    for k in trunk + never:
        assert torch.equal(c["net"][k], init[k]), k
    assert all(not torch.equal(c["net"][k], init[k]) for k in top)
    # the optimiser state: exactly the stepped tensors, at their parameter indices
    index = {e["name"]: i for i, e in enumerate(src._table)}
    assert sorted(c["optimizer"]["state"]) == sorted(index[k] for k in top)
    assert c["epoch"] == 2 and float(next(iter(c["optimizer"]["state"].values()))["step"]) == 8.0
    assert np.isfinite(float(c["last_val_loss"]))
    # the checkpoint loads into both model classes (the other task's class takes everything but the last layer of the head)
    Model().load_state_dict(c["net"])
    Other = ChromoformerClassifier if reg else ChromoformerRegressor
    Other().load_state_dict({k: v for k, v in c["net"].items() if not k.startswith("fc_head.2.")}, strict=False)
