"""Host-only checks of the frozen-trunk feature: the new ABI symbols and their ctypes signatures, the frozen / stepped partition of the
parameter layout, the warm start of `train --init-from` (key modernisation, refusals), argument parsing and the sweep's pass-through,
the optimiser state a frozen-trunk checkpoint carries.  No compute call is made."""
import ctypes as C
import os
import re

import pytest
import torch

from chromoformer_amd import _lib
from tests.test_abi_cpu import _cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cf_trunk_outputs", "cf_forward_train_x0", "cf_x0_gather", "cf_x0_gather_fwd", "cf_reduce_opt_x0", "cf_backward_from_top")


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"^int %s\(cf_handle\* h," % name, hdr, re.M), name
        assert hasattr(L, name) and name in _lib.SYMBOLS
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[0] is C.c_void_p
        # one ctypes argument per parameter of the declaration
        decl = re.search(r"^int %s\((.*?)\);" % name, hdr, re.M | re.S).group(1)
        assert len(args) == decl.count(",") + 1, (name, decl)
    assert _lib.SYMBOLS["cf_forward_train_x0"][1][5] is C.c_float                      # loss_scale
    assert _lib.SYMBOLS["cf_reduce_opt_x0"][1][2:7] == [C.c_float] * 5 and _lib.SYMBOLS["cf_reduce_opt_x0"][1][7] is C.c_longlong
    assert _lib.SYMBOLS["cf_x0_gather"][1][1] == C.POINTER(_lib.cf_x0_store)
    # cf_x0_store mirrors the header: n_genes, x0[3], interaction_mask[3], interaction_freq, labels
    assert [f[0] for f in _lib.cf_x0_store._fields_] == ["n_genes", "x0", "interaction_mask", "interaction_freq", "labels"]
    assert C.sizeof(_lib.cf_x0_store) == 8 + 3 * 8 + 3 * 8 + 8 + 8
    # the version stays 1 although symbols were added: tests/test_abi_cpu.py asserts 1, and so do _lib.lib()
    # and the package's build(); the additions leave every existing symbol and struct as it was
    assert L.cf_abi_version() == 1
    # host-side refusals that need no device
    assert L.cf_trunk_outputs(None, None, None, None) != 0 and b"cf_trunk_outputs" in L.cf_last_error()
    assert L.cf_forward_train_x0(None, None, None, None, None, 1.0, None, None) != 0 and b"cf_forward_train_x0" in L.cf_last_error()
    assert L.cf_x0_gather(None, None, None, None, None, None, None) != 0 and b"cf_x0_gather" in L.cf_last_error()
    assert L.cf_reduce_opt_x0(None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, None, None) != 0 and b"cf_reduce_opt_x0" in L.cf_last_error()


@pytest.mark.parametrize("n_out", [2, 1])
def test_the_frozen_and_stepped_partition_is_the_two_buckets(n_out):
    from chromoformer_amd.net import is_trunk_name, split_layout
    lay, tab = _lib.param_layout(_cfg(n_out))
    trunk, top, never = split_layout(tab)
    by = {t["name"]: t for t in tab}
    assert len(never) == 36 and len(trunk) + len(top) + len(never) == lay.n_tensors
    assert all(n.startswith(("embed.", "pairwise_interaction.")) for n in trunk)
    assert all(n.startswith(("regulation.", "fc_head.")) for n in top)
    assert {n for n in by if n.startswith(("embed.", "pairwise_interaction.")) and by[n]["trainable"]} == set(trunk)
    assert {n for n in by if n.startswith(("regulation.", "fc_head."))} - set(never) == set(top)
    # two adjacent ranges of the flat buffers: [0, split) = CF_BUCKET_PE, [split, n_active) = CF_BUCKET_REG; the rest is never stepped
    span = lambda names: (min(by[n]["offset"] for n in names), max(by[n]["offset"] + by[n]["numel"] for n in names))
    (t0, t1), (r0, r1), (z0, _) = span(trunk), span(top), span(never)
    assert t0 == 0 and t1 <= r0 and r0 - t1 < 4 and r1 <= lay.n_active <= z0
    assert not any(is_trunk_name(n) for n in top) and all(is_trunk_name(n) for n in trunk)


@pytest.mark.parametrize("n_out", [2, 1])
def test_checkpoint_optimiser_state_carries_exactly_the_stepped_tensors(n_out):
    from chromoformer_amd.net import split_layout
    from chromoformer_amd.train import stepped_indices
    _, tab = _lib.param_layout(_cfg(n_out))
    trunk, top, never = split_layout(tab)
    full, frozen = stepped_indices(tab), stepped_indices(tab, freeze_trunk=True)
    assert len(full) == len(trunk) + len(top) == len(tab) - len(never)
    assert [tab[i]["name"] for i in frozen] == top and set(frozen) < set(full)
    assert not {tab[i]["name"] for i in frozen} & set(trunk + never)


def _model():
    from chromoformer_amd import ChromoformerClassifier
    return ChromoformerClassifier(seed=3)


def test_init_from_loads_current_legacy_and_bare_state_dicts(tmp_path):
    from chromoformer_amd import Chromoformer
    from chromoformer_amd.train import load_init_weights
    src = _model()
    want = {k: v.clone() for k, v in src.state_dict().items()}
    legacy = Chromoformer(seed=3).state_dict()                      # `embed2000.` / `pw_int2000.` / `reg2000.` keys
    assert any(k.startswith("pw_int2000.") for k in legacy)
    for name, obj in (("ckpt", {"net": src.state_dict(), "optimizer": {"state": {0: {"step": torch.tensor(5.0)}}}, "epoch": 3}),
                      ("bare", dict(src.state_dict())), ("legacy", {"net": legacy})):
        path = str(tmp_path / (name + ".pt"))
        torch.save(obj, path)
        dst = type(src)(seed=11)
        assert not torch.equal(dst.state_dict()["fc_head.0.weight"], want["fc_head.0.weight"])
        load_init_weights(dst, path)
        got = dst.state_dict()
        assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want), name
        assert dst._step == 0                                       # a warm start, not a resume


def test_init_from_refusals(tmp_path):
    from chromoformer_amd import ChromoformerClassifier
    from chromoformer_amd.train import load_init_weights
    sd = dict(_model().state_dict())
    path = str(tmp_path / "c.pt")
    key = "regulation.500.transformer.layers.2.ff.l1.weight"
    torch.save({k: v for k, v in sd.items() if k != key}, path)
    with pytest.raises(KeyError, match=re.escape(key)):
        load_init_weights(_model(), path)
    torch.save(dict(sd, **{"regulation.500.extra.weight": torch.zeros(1)}), path)
    with pytest.raises(KeyError, match="regulation.500.extra.weight"):
        load_init_weights(_model(), path)
    torch.save(sd, path)
    other = ChromoformerClassifier(regulation_kws={"n_layers": 6, "n_heads": 8, "d_model": 256, "d_ff": 128})
    with pytest.raises(ValueError, match="shape mismatch at `regulation.2000.transformer.layers.0.ff.l1.weight`"):
        load_init_weights(other, path)
    torch.save({"epoch": 1}, path)
    with pytest.raises(ValueError, match="neither a checkpoint"):
        load_init_weights(_model(), path)


def test_arguments_and_sweep_pass_through():
    from chromoformer_amd import sweep, train
    base = ["-o", "o.pt", "-c", "c.yaml", "--exp-id", "e", "-m", "m.csv", "-d", "npy", "--fold", "0"]
    a = train.build_parser().parse_args(base)
    assert a.init_from is None and a.freeze_trunk is False
    a = train.build_parser().parse_args(base + ["--init-from", "ck.pt", "--freeze-trunk"])
    assert a.init_from == "ck.pt" and a.freeze_trunk is True
    sw = ["--meta-template", "d/{eid}/train.csv", "--npy-dir-template", "d/{eid}/npy", "-c", "c.yaml"]
    plain = sweep.command("E003", "4", "o.pt", sweep.build_parser().parse_args(sw))
    assert "--init-from" not in plain and "--freeze-trunk" not in plain
    cmd = sweep.command("E003", "4", "o.pt", sweep.build_parser().parse_args(sw + ["--init-from", "ck/E116-fold{fold}.pt", "--freeze-trunk"]))
    assert cmd[: len(plain)] == plain and cmd[len(plain):] == ["--init-from", "ck/E116-fold4.pt", "--freeze-trunk"]
    # what the sweep emits is what the trainer parses
    t = train.build_parser().parse_args(cmd[3:])
    assert t.init_from == "ck/E116-fold4.pt" and t.freeze_trunk and t.fold == 0


def test_freeze_granularity_is_named():
    from chromoformer_amd.net import FREEZE_GRANULARITY
    m = _model()
    assert m._trunk_frozen() is False
    m.freeze_trunk()
    assert m._trunk_frozen() is True
    named = dict(m.named_parameters())
    named["embed.100.lin_proj.weight"].requires_grad_(True)
    with pytest.raises(RuntimeError) as e:
        m._trunk_frozen()
    assert "embed.100.lin_proj.weight" in str(e.value) and FREEZE_GRANULARITY in str(e.value)
    m.freeze_trunk(False)
    named["fc_head.0.bias"].requires_grad_(False)
    with pytest.raises(RuntimeError, match="fc_head.0.bias"):
        m._trunk_frozen()
