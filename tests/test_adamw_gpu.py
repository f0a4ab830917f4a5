"""Every launch path of the AdamW update (adamw_elem, csrc/cf_kernels.h) against torch.optim.AdamW's formula in float64, element by
element: parameters, exp_avg and exp_avg_sq, inside the rounding bounds of tests/adamw_reference.py.  No oracle gradient is involved --
the optimiser is handed known gradients, or its own are read back -- so the tolerances are a few units of fp32 rounding.

  a. cf_adamw_step (k_adamw) on a prescribed adversarial state, seven hyper-parameter sets, a model under one grid sweep and one that
     takes the grid-stride loop; nothing at or beyond n_active is written, the gradients are never written
  b. every legal bucket mask of cf_adamw_step_part: inside the range within bounds, outside it bit-unchanged; the refusals
  c. k_adamw_tiled: the tiled copies it writes give the logits of tiles built from scratch
  d. through the Trainer on the device's own gradients, every single-GPU schedule (separate launches, k_reduce_adamw, the reduction
     epilogues, riders, hipGraph replay, the frozen trunk), non-default hyper-parameters, a decaying learning rate, 12 steps, and a leg at
     step 10^6; all non-frozen schedules bit-equal
  e. the exported optimiser state loads into torch.optim.AdamW and steps there to the same reference

Worst |d| / bound measured on an MI355X (1.0 is the bound; in units of u = 2^-24 multiply p by 8, m and v by 4), over all launch paths:
p 0.669 (5.4 u), m 0.257 (1.0 u), v 0.486 (1.9 u), all three on the adversarial state through k_adamw; on the Trainer's own gradients
p 0.42, m 0.25, v 0.47 on every path.  Per launch path: MEASURED below.  torch.optim.AdamW in fp32 on the CPU: 0.52 / 0.23 / 0.39."""
import ctypes as C

import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.adamw_reference import HYPER_SETS, adversarial_state, bounds, f32, reference, worst_ratios
from tests.helpers import build_model
from tests.test_config_variants_gpu import VARIANTS

pytestmark = pytest.mark.gpu

#: worst |d| / bound (p, m, v) per launch path as measured on an MI355X (gfx950); the tests print theirs on every run.  The non-frozen
#: Trainer schedules are bit-equal, hence the equal figures (default model; odd_lengths: p 0.407, frozen p 0.422).
MEASURED = {
    "k_adamw, cf_adamw_step, seven hyper-parameter sets": (0.669, 0.257, 0.486),        # = 5.4 u, 1.0 u, 1.9 u
    "k_adamw, the bucket masks of cf_adamw_step_part": (0.445, 0.248, 0.451),
    "k_adamw_tiled": (0.460, 0.248, 0.435),
    "Trainer separate (k_adamw)": (0.398, 0.249, 0.472),
    "Trainer merged (k_reduce_adamw + k_adamw)": (0.398, 0.249, 0.472),
    "Trainer fused, no riders (k_reduce_opt epilogues)": (0.398, 0.249, 0.472),
    "Trainer fused, riders (37 / 100000 tiles, 512 under replay)": (0.398, 0.249, 0.472),
    "Trainer frozen trunk (k_reduce_opt_x0)": (0.343, 0.249, 0.472),
    "Trainer fused under replay from step 10^6": (0.350, 0.249, 0.472),
    "exported state, step 6, library": (0.302, 0.247, 0.471),
    "exported state, step 6, torch.optim.AdamW fp32 on the CPU": (0.307, 0.227, 0.471),
}

ARGS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
MODELS = {"tiny": dict(VARIANTS["shallow_narrow"], i_max=2), "default": None, "odd_lengths": VARIANTS["odd_lengths"]}
PE, REG, REG_HI, REG_LO = 2, 1, 4, 8
MASK_NAMES = {PE: "PE", REG: "REG", REG_LO: "REG_LO", REG_HI: "REG_HI", PE | REG_LO: "PE|REG_LO", REG_LO | REG_HI: "REG_LO|REG_HI", PE | REG: "PE|REG"}
# the Trainer legs run on hyper-parameters that are fp32 numbers already: the library, torch and the reference see the same values
LR, BETAS, EPS, WD = f32(1e-3), (f32(0.8), f32(0.95)), f32(1e-4), f32(0.1)
HP_MASKS = HYPER_SETS[2]
_cache = {}


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _state(n):
    """The first n elements of ONE adversarial state on the device (the patterns depend on the index only), never written."""
    if "state" not in _cache:
        n_max = max(build_layout(k).n_total for k in ("tiny", "default"))
        _cache["state"] = adversarial_state(n_max, 20240607, "cuda:0")
    return tuple(t[:n] for t in _cache["state"])


def build_layout(name):
    from chromoformer_amd import _lib
    c = orc._cfg(MODELS[name])
    cfg = _lib.make_config(c["n_feats"], c["d_emb"], c["d_head"], 2, c["binsizes"], [c["w_max"] // b for b in c["binsizes"]], c["i_max"],
                           c["embed"], c["pairwise_interaction"], c["regulation"], 4)
    return _lib.param_layout(cfg)[0]


def _model(name, B=4):
    return build_model(orc._cfg(MODELS[name]), False, B)


def _buckets(model):
    from chromoformer_amd import _lib
    out = {}
    for b in (PE, REG, REG_LO, REG_HI):
        off, n = C.c_longlong(), C.c_longlong()
        _lib.check(_lib.lib().cf_grad_bucket(model._handle, b, C.byref(off), C.byref(n)), "cf_grad_bucket")
        out[b] = (off.value, off.value + n.value)
    out[PE | REG_LO] = (out[PE][0], out[REG_LO][1])
    out[REG_LO | REG_HI] = out[REG]
    out[PE | REG] = (out[PE][0], out[REG][1])
    return out


def _fill(model, what="pgmv"):
    """Every element of the flat buffers from the adversarial state, the never-trained tail beyond n_active included ("gmv": the
    parameters stay, and the library is not told of a change)."""
    n = model._flat.numel()
    p, g, m, v = _state(n)
    with torch.no_grad():
        if "p" in what:
            model._flat.copy_(p)
            model.params_changed()
        model._gflat.copy_(g)
        model._mflat.copy_(m)
        model._vflat.copy_(v)
    torch.cuda.synchronize()
    return model._flat.clone(), g, m, v


def _snapshot(model):
    torch.cuda.synchronize()
    return model._flat.clone(), model._mflat.clone(), model._vflat.clone()


def _check_range(model, before, g, hp, lo, hi, what):
    """(p, m, v) of the model over [lo, hi) against the reference of `before` (p, m, v clones) and g; everything else bit-unchanged.
    -> worst ratios [p, m, v]."""
    torch.cuda.synchronize()
    after = (model._flat, model._mflat, model._vflat)
    p0, m0, v0 = (t[lo:hi] for t in before)
    got = tuple(t[lo:hi] for t in after)
    assert all(bool(torch.isfinite(t).all()) for t in got), what
    worst = worst_ratios(got, reference(p0, g[lo:hi], m0, v0, *hp), bounds(p0, g[lo:hi], m0, v0, *hp))
    for a, b, k in zip(after, before, "pmv"):
        assert _same_bits(a[:lo], b[:lo]) and _same_bits(a[hi:], b[hi:]), (what, k, "written outside [%d, %d)" % (lo, hi))
    return worst


def _report(path, worst, what=""):
    print("AdamW %-34s worst |d| / bound  p %.3f  m %.3f  v %.3f  %s" % (path, *worst, what))


def _step_part(model, hp, mask=None):
    from chromoformer_amd import _lib
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    lr, b1, b2, eps, wd, step = hp
    if mask is None:
        return L.cf_adamw_step(model._handle, lr, b1, b2, eps, wd, step, st)
    return L.cf_adamw_step_part(model._handle, lr, b1, b2, eps, wd, step, mask, st)


# ----------------------------------------------------------------------------- a. operator level, prescribed state
@pytest.mark.parametrize("name", ["tiny", "default"])
def test_adamw_step_on_a_prescribed_state(name):
    model = _model(name)
    lay = model._layout
    n4 = lay.n_active // 4
    assert lay.n_active % 4 == 0 and lay.n_total > lay.n_active
    if name == "tiny":      # under one sweep of the 2048 x 256 grid, the last block partly filled
        assert n4 < 2048 * 256 and n4 % 256
    else:                   # the grid-stride loop runs
        assert n4 > 2048 * 256
    overall = [0.0, 0.0, 0.0]
    for hp in HYPER_SETS:
        p0, g, m0, v0 = _fill(model)
        g0 = model._gflat.clone()
        assert _step_part(model, hp) == 0
        worst = _check_range(model, (p0, m0, v0), g, hp, 0, lay.n_active, (name, hp))
        assert _same_bits(model._gflat, g0), (name, hp, "the gradients were written")
        _report("k_adamw %s" % name, worst, str(hp))
        assert max(worst) <= 1.0, (name, hp, worst)
        overall = [max(a, b) for a, b in zip(overall, worst)]
    print("AdamW k_adamw %s: worst over the hyper-parameter sets  p %.3f  m %.3f  v %.3f" % (name, *overall))


# ----------------------------------------------------------------------------- b. bucket masks
@pytest.mark.parametrize("name", ["tiny", "default"])
def test_bucket_masks_step_their_range_and_nothing_else(name):
    model = _model(name)
    bk = _buckets(model)
    n_active = model._layout.n_active
    assert bk[PE][0] == 0 and bk[PE][1] == bk[REG_LO][0] and bk[REG_LO][1] == bk[REG_HI][0] and bk[REG_HI][1] == n_active
    hp = HP_MASKS
    for mask, (lo, hi) in sorted(bk.items()):
        p0, g, m0, v0 = _fill(model)
        assert _step_part(model, hp, mask) == 0, MASK_NAMES[mask]
        worst = _check_range(model, (p0, m0, v0), g, hp, lo, hi, (name, MASK_NAMES[mask]))
        _report("k_adamw %s mask %s" % (name, MASK_NAMES[mask]), worst, "[%d, %d)" % (lo, hi))
        assert max(worst) <= 1.0, (name, MASK_NAMES[mask], worst)
    # the three buckets one after the other: the bits of one launch over everything
    _fill(model)
    assert _step_part(model, hp) == 0
    whole = _snapshot(model)
    _fill(model)
    for mask in (PE, REG_LO, REG_HI):
        assert _step_part(model, hp, mask) == 0
    for a, b, k in zip(_snapshot(model), whole, "pmv"):
        assert _same_bits(a, b), (name, k)


def test_bucket_mask_and_step_refusals_leave_the_buffers_alone():
    from chromoformer_amd import _lib
    model = _model("tiny")
    L = _lib.lib()
    _fill(model)
    before = _snapshot(model) + (model._gflat.clone(),)
    lr, b1, b2, eps, wd, step = HP_MASKS
    for mask, st_, text in ((PE | REG_HI, step, b"not adjacent"), (0, step, b"bad bucket mask"), (16, step, b"bad bucket mask"),
                            (PE | 32, step, b"bad bucket mask"), (PE, 0, b"1-based"), (PE | REG, -3, b"1-based")):
        assert _step_part(model, (lr, b1, b2, eps, wd, st_), mask) != 0, (mask, st_)
        assert text in L.cf_last_error(), (mask, st_, L.cf_last_error())
    assert _step_part(model, (lr, b1, b2, eps, wd, 0)) != 0 and b"1-based" in L.cf_last_error()
    for a, b, k in zip(_snapshot(model) + (model._gflat,), before, "pmvg"):
        assert _same_bits(a, b), k


# ----------------------------------------------------------------------------- c. k_adamw_tiled
def test_tiled_copies_written_by_the_optimiser_equal_tiles_built_from_scratch():
    """The model's own (seeded) weights, adversarial gradients and moments: the PE bucket stepped alone under keep_tiled goes through
    k_adamw_tiled, and the next forward pass reads the tiled copies that launch wrote."""
    from chromoformer_amd import _lib
    model = _model("default")
    assert model.keep_tiled(True)
    batch = orc.synthetic_batch(3, seed=5, regime="realistic")
    with torch.no_grad():
        model(*[batch[k] for k in ARGS])           # (the first pass builds every tiled copy; later ones skip the PE tensors while they are fresh)
    p0, g, m0, v0 = _fill(model, "gmv")            # (nothing tells the library of a change: no re-tiling in front of the next pass)
    lo, hi = _buckets(model)[PE]
    assert _step_part(model, HP_MASKS, PE) == 0
    worst = _check_range(model, (p0, m0, v0), g, HP_MASKS, lo, hi, "k_adamw_tiled")
    _report("k_adamw_tiled", worst)
    assert max(worst) <= 1.0, worst
    assert not _same_bits(model._flat[lo:hi], p0[lo:hi])
    with torch.no_grad():
        logits = model(*[batch[k] for k in ARGS]).clone()
        n_fwd = model.launch_counts()[0]
        _lib.check(_lib.lib().cf_params_changed(model._handle), "cf_params_changed")      # ... and now with the copies rebuilt by the pass: one launch more, the same bits
        again = model(*[batch[k] for k in ARGS]).clone()
        assert model.launch_counts()[0] == n_fwd + 1, "the pass behind the optimiser launch re-tiled: it did not read what k_adamw_tiled wrote"
    assert _same_bits(logits, again)
    fresh = _model("default")
    fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
    with torch.no_grad():
        ref = fresh(*[batch[k] for k in ARGS])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(logits).all()) and _same_bits(logits, ref), (logits, ref)


# ----------------------------------------------------------------------------- d. through the Trainer, on the device's own gradients
SCHEDULES = {
    "separate": dict(use_graph=False, merge_opt=False),
    "merged": dict(merge_opt=True, fuse_opt=False),
    "fused_riders_0": dict(fuse_opt=True, keep_grads=True, rider_tiles=0),
    "fused_riders_37": dict(fuse_opt=True, keep_grads=True, rider_tiles=37),
    "fused_riders_100000": dict(fuse_opt=True, keep_grads=True, rider_tiles=100000),
    "fused_graph": dict(use_graph=True, fuse_opt=True, keep_grads=True),
    "frozen": dict(freeze_trunk=True, keep_grads=True),
}


def _leg(name, sched, steps=12, first_step=0):
    """`steps` Trainer steps at B = 4 over two alternating batches, gamma = 0.5 applied after steps 4 and 8; every step checked against the
    reference of the state cloned in front of it and the gradients read back behind it.  -> (model, trainer, slots, worst, losses)."""
    from chromoformer_amd.engine import Trainer
    cfg = orc._cfg(MODELS[name])
    model = _model(name)
    model._step = first_step
    tr = Trainer(model, lr=LR, gamma=0.5, betas=BETAS, eps=EPS, weight_decay=WD, **SCHEDULES[sched])
    frozen = SCHEDULES[sched].get("freeze_trunk", False)
    lo, hi = _buckets(model)[REG] if frozen else (0, model._layout.n_active)
    slots = [tr.stage(orc.synthetic_batch(4, cfg=cfg, seed=31 + i, regime="realistic")) for i in range(2)]
    worst, losses = [0.0, 0.0, 0.0], []
    for i in range(steps):
        before = _snapshot(model)
        hp = (tr.lr, BETAS[0], BETAS[1], EPS, WD, model._step + 1)
        _, loss = tr.step(slots[i % 2])
        torch.cuda.synchronize()
        losses.append(float(loss))
        assert model._step == first_step + i + 1
        w = _check_range(model, before, model._gflat, hp, lo, hi, (name, sched, i))      # (frozen: the PE range and the tail bit-unchanged)
        assert max(w) <= 1.0, (name, sched, "step %d" % (i + 1), w)
        assert not _same_bits(model._flat[lo:hi], before[0][lo:hi])
        worst = [max(a, b) for a, b in zip(worst, w)]
        if i + 1 in (4, 8):
            tr.scheduler_step()
    assert steps < 12 or tr.lr == LR * 0.25
    return model, tr, slots, worst, losses


def _final(model, losses):
    return tuple(t.clone() for t in (model._flat, model._mflat, model._vflat)) + (losses,)


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("name", ["default", "odd_lengths"])
def test_trainer_steps_lie_inside_the_bounds_of_their_own_gradients(name, sched):
    model, tr, _, worst, losses = _leg(name, sched)
    _report("Trainer %s" % sched, worst, name)
    if sched.startswith("fused"):
        assert tr.fuse_opt and (tr.rider_tiles > 0) == (sched != "fused_riders_0"), (tr.fuse_opt, tr.rider_tiles)
    if sched == "frozen":
        return
    # all non-frozen schedules end on the same bits
    key = ("final", name)
    if key not in _cache:
        if sched == "separate":
            _cache[key] = _final(model, losses)
        else:
            ref_model, _, _, _, ref_losses = _leg(name, "separate")
            _cache[key] = _final(ref_model, ref_losses)
    ref = _cache[key]
    assert losses == ref[3], (name, sched)
    for a, b, k in zip(_final(model, losses), ref, "pmv"):
        assert _same_bits(a, b), (name, sched, k)


@pytest.mark.parametrize("name", ["default", "odd_lengths"])
def test_trainer_steps_at_step_one_million(name):
    """beta^step underflows to 0: both bias corrections are exactly 1."""
    _, _, _, worst, _ = _leg(name, "fused_graph", first_step=10 ** 6 - 1)
    _report("Trainer fused_graph step 1e6", worst, name)


# ----------------------------------------------------------------------------- e. exported state
@pytest.mark.parametrize("frozen", [False, True])
def test_exported_state_loads_into_torch_adamw_and_steps_to_the_same_reference(frozen):
    from chromoformer_amd import train
    from chromoformer_amd.net import is_trunk_name
    model, tr, slots, _, _ = _leg("default", "frozen" if frozen else "fused_graph", steps=5)
    lr = tr.lr
    sd = train.optimizer_state_dict(model, lr, betas=BETAS, eps=EPS, weight_decay=WD, freeze_trunk=frozen)
    table = model._table
    stepped = [i for i, e in enumerate(table) if e["trainable"] and not (frozen and is_trunk_name(e["name"]))]
    assert [n for n, _ in model.named_parameters()] == [e["name"] for e in table]
    # key set, shapes and step; never-trained (and frozen) parameters have no entry
    assert sorted(sd["state"]) == stepped == train.stepped_indices(table, frozen) and len(stepped) < len(table)
    for i in stepped:
        st = sd["state"][i]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 5.0 and st["step"].dtype == torch.float32
        assert tuple(st["exp_avg"].shape) == tuple(st["exp_avg_sq"].shape) == tuple(table[i]["shape"]), table[i]["name"]
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
    torch.optim.AdamW(model.parameters(), **kw).load_state_dict(sd)
    # one more step both ways: torch in float32 on CPU copies, the library on the device, the gradients the library published
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in model.parameters()]
    opt = torch.optim.AdamW(cpu, **kw)
    opt.load_state_dict(sd)
    grp = opt.param_groups[0]
    assert (grp["lr"], tuple(grp["betas"]), grp["eps"], grp["weight_decay"]) == (lr, BETAS, EPS, WD)      # what the run stepped with travels with the state
    before = _snapshot(model)
    tr.step(slots[1])
    torch.cuda.synchronize()
    g = model._gflat.clone()
    hp = (lr, BETAS[0], BETAS[1], EPS, WD, 6)
    lo, hi = _buckets(model)[REG] if frozen else (0, model._layout.n_active)
    w_lib = _check_range(model, before, g, hp, lo, hi, "library")
    g_cpu = g.cpu()
    for i in stepped:
        e = table[i]
        cpu[i].grad = g_cpu[e["offset"]:e["offset"] + e["numel"]].view(e["shape"])
    opt.step()
    assert sorted(opt.state_dict()["state"]) == stepped
    flat_t = [t.cpu().clone() for t in before]
    for i, e in enumerate(table):
        sl = slice(e["offset"], e["offset"] + e["numel"])
        if i not in sd["state"]:      # never trained (or frozen): no state, and it does not move -- on either side
            assert torch.equal(cpu[i].detach().reshape(-1), flat_t[0][sl]), e["name"]
            assert _same_bits(model._flat[sl], before[0][sl]), e["name"]
            continue
        st = opt.state[cpu[i]]
        assert float(st["step"]) == 6.0
        flat_t[0][sl], flat_t[1][sl], flat_t[2][sl] = cpu[i].detach().reshape(-1), st["exp_avg"].reshape(-1), st["exp_avg_sq"].reshape(-1)
    p0, m0, v0 = (t[lo:hi] for t in before)
    ref, bnd = reference(p0, g[lo:hi], m0, v0, *hp), bounds(p0, g[lo:hi], m0, v0, *hp)
    w_torch = worst_ratios(tuple(t.cuda()[lo:hi] for t in flat_t), ref, bnd)
    _report("exported state, library step 6", w_lib, "frozen" if frozen else "")
    _report("exported state, torch step 6", w_torch, "frozen" if frozen else "")
    assert max(w_lib) <= 1.0 and max(w_torch) <= 1.0, (w_lib, w_torch)
