"""The contact games, host side (no GPU): the rule of include/chromoformer_hip.h as tests/contact_oracle.py states it against the
reference's logits (tests/golden/contact_games.npz), attribution.contact_players, and the three facts the rule implies, each exactly,
on the CPU oracle:

  * a game whose players only drop is the pCRE game (tests/coalition_oracle.coalition_masks, every tensor bit-equal);
  * a masked score is replaced, not biased: next to a dropped slot j its contact is a null player;
  * scale = 1, a donor equal to the gene's own frequencies and a dummy slot are null players;

and the efficiency of the float64 Shapley values of the oracle's table."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.coalition_oracle import coalition_masks, shapley_fp64
from tests.contact_oracle import contact_batch, gone_words, oracle_contact_coalitions
from tests.helpers import GOLDEN, load_npz_batch

TOL = 1e-4      # the project's logit bound
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _players(spec, S):
    from chromoformer_amd.attribution import contact_players
    return contact_players(spec, S)


def test_oracle_reproduces_the_reference_goldens():
    """A sample of every recorded game (the generator checked all of them to 1e-5 before it wrote the file)."""
    z = np.load(os.path.join(GOLDEN, "contact_games.npz"))
    assert z["contacts0.clf"].shape == (6, 256, 2) and z["joint.clf"].shape == (6, 32, 2) and z["donor.reg"].shape == (6, 32, 1)
    batch = {k: v for k, v in load_npz_batch("demo_subset.npz")[0].items() if k != "label"}
    donor = torch.roll(batch["interaction_freq"], 1, 0)
    contacts, joint = _players("contacts", 8), _players("pcres_and_contacts", 8)
    P = {False: orc.init_params(None, 42, False), True: orc.init_params(None, 42, True)}
    words8, words16 = z["words8"], z["joint.words"]
    assert int(words8[0]) == 255 and int(words8[1]) == 0 and int(words16[0]) == 0xFFFF and int(words16[1]) == 0
    cases = [("contacts0.clf", contacts, np.arange(256), [255, 0, 1, 0x80, 0x5A, 0xA5, 0x0F, 0xF7], 0.0, None, False),
             ("joint.clf", joint, words16, range(8), 0.0, None, False), ("joint.reg", joint, words16, range(8, 12), 0.0, None, True),
             ("half.clf", contacts, words8, range(4), 0.5, None, False), ("half.reg", contacts, words8, range(4, 8), 0.5, None, True),
             ("donor.clf", contacts, words8, range(4), 0.0, donor, False), ("donor.reg", contacts, words8, range(4, 8), 0.0, donor, True)]
    for name, (drop, contact, _), words, cols, scale, don, regression in cases:
        cols = list(cols)
        got = oracle_contact_coalitions(P[regression], batch, [int(words[c]) for c in cols], drop, contact, scale, don).numpy()
        d = np.abs(got - z[name][:, cols]).max()
        print("%s: oracle vs the reference %.3e" % (name, d))
        assert d < TOL, (name, d)
    # the games differ: the recorded rows are not one table under several names
    assert np.abs(z["half.clf"] - z["donor.clf"])[:, 2:].max() > 1e-3
    assert np.abs(z["half.clf"][:, 1] - z["contacts0.clf"][:, 0]).max() > 1e-3      # nobody at scale 0.5 is not nobody at scale 0
    assert np.array_equal(z["half.clf"][:, 0], z["contacts0.clf"][:, 255])           # everybody is the prediction in every game


def test_contact_players_specs_names_and_refusals():
    from chromoformer_amd.attribution import CONTACT_PLAYER_SPECS, contact_players
    assert CONTACT_PLAYER_SPECS == ("contacts", "pcres", "pcres_and_contacts", "all")
    d, c, n = contact_players("contacts", 8)
    assert d.dtype == c.dtype == np.uint32 and d.tolist() == [0] * 8 and c.tolist() == [1 << j for j in range(8)]
    assert n == ["contact%d" % j for j in range(8)]
    d, c, n = contact_players("pcres", 5)
    assert d.tolist() == [1, 2, 4, 8, 16] and c.tolist() == [0] * 5 and n == ["pcre%d" % j for j in range(5)]
    d, c, n = contact_players("pcres_and_contacts", 3)
    assert d.tolist() == [1, 2, 4, 0, 0, 0] and c.tolist() == [0, 0, 0, 1, 2, 4]
    assert n == ["pcre0", "pcre1", "pcre2", "contact0", "contact1", "contact2"]
    assert len(contact_players("pcres_and_contacts", 8)[2]) == 16
    d, c, n = contact_players("all", 16)
    assert d.tolist() == [0] and c.tolist() == [0xFFFF] and n == ["contacts"]
    d, c, n = contact_players([([0, 2], [1]), ((), (3, 3, 0)), ([1], [])], 4)      # overlapping players, a generator-free list form
    assert d.tolist() == [5, 0, 2] and c.tolist() == [2, 9, 0] and len(n) == 3 and len(set(n)) == 3
    assert len(contact_players("contacts", 16)[2]) == 16
    with pytest.raises(ValueError, match="contact_players.*i_max = 9 > 8.*'contacts'.*list of"):
        contact_players("pcres_and_contacts", 9)
    for bad, needle in (("marks", "choose from"), ([([], [])], "player 0 is empty"), ([([4], [])], r"drop slot\(s\) \[4\] outside"),
                        ([([], [-1])], r"contact slot\(s\) \[-1\] outside"), ([], "0 players"), ([([0], [])] * 17, "17 players"),
                        ([3], "list of"), ([("a", [0])], "list of")):
        with pytest.raises(ValueError, match="contact_players: .*" + needle):
            contact_players(bad, 4)


def test_drop_only_players_give_the_pcre_game_bit_for_bit():
    S = 8
    batch = orc.synthetic_batch(4, seed=31, regime="realistic")
    drop, contact, _ = _players("pcres", S)
    for m in (255, 0, 1, 0x5A, 0xF7, 0x80):
        a, b = contact_batch(batch, m, drop, contact, scale=0.0), coalition_masks(batch, m, S)
        for k, v in a.items():
            for x, y in (zip(v.values(), b[k].values()) if isinstance(v, dict) else [(v, b[k])]):
                assert torch.equal(x, y), (hex(m), k)
    # the rule's words: D and C of a coalition, overlapping players OR-ed, an entry named twice edited once
    assert gone_words(0b01, [1, 2], [4, 8]) == (2, 8) and gone_words(0, [1, 3], [4, 4]) == (3, 4) and gone_words(3, [1, 2], [4, 8]) == (0, 0)
    dense = dict(batch, interaction_freq=torch.arange(4 * 81, dtype=torch.float32).reshape(4, 9, 9) + 1)
    e = contact_batch(dense, 0, [0, 0], [0b011, 0b110], scale=0.5)["interaction_freq"]      # slots 0, 1 | 1, 2: rows and columns 1..3
    hit = torch.zeros(9, 9, dtype=torch.bool)
    hit[1:4, :] = True
    hit[:, 1:4] = True
    assert torch.equal(e[:, hit], 0.5 * dense["interaction_freq"][:, hit]) and torch.equal(e[:, ~hit], dense["interaction_freq"][:, ~hit])
    assert not bool(hit[0, 0]) and bool(hit[0, 1]) and bool(hit[1, 0]) and bool(hit[5, 2])


@pytest.fixture(scope="module")
def small():
    """i_max = 3, 5 genes with [0, 0, 0, 2, 3] dummy slots, dense signed frequencies (so that rows >= 1 and columns matter), the joint
    game's 64 rows by the oracle (computed once)."""
    cfg = orc._cfg(dict(i_max=3))
    batch = orc.synthetic_batch(5, cfg=cfg, seed=13, regime="realistic")
    batch["interaction_freq"] = torch.from_numpy(np.random.default_rng(5).normal(0.0, 1.5, size=(5, 4, 4)).astype(np.float32))
    P = orc.init_params(cfg, 3, False)
    drop, contact, names = _players("pcres_and_contacts", 3)
    return cfg, batch, P, (drop, contact, names), oracle_contact_coalitions(P, batch, range(64), drop, contact, 0.0, None, cfg)


def test_next_to_a_dropped_slot_its_contact_is_null_exactly(small):
    cfg, batch, P, (drop, contact, names), rows = small
    dummy = torch.stack([m[:, 0, 0, 1:] for m in batch["interaction_masks"].values()]).all(0)
    assert dummy.sum(1).tolist() == [0, 0, 0, 2, 3]
    differs = 0
    for j in range(3):
        for m in range(64):
            if m >> j & 1 or m >> (3 + j) & 1:
                continue      # m: pcre j absent, contact j absent
            assert torch.equal(rows[:, m], rows[:, m | 1 << (3 + j)]), (j, m)
            both = rows[:, m | 1 << j | 1 << (3 + j)]      # with pcre j present the contact bit matters for live slots ...
            live = ~dummy[:, j]
            differs += int(not torch.equal(both[live], rows[live, m | 1 << j]))
            assert torch.equal(both[~live], rows[~live, m | 1 << j])      # ... and a dummy slot's players are null
            assert torch.equal(rows[~live, m], rows[~live, m | 1 << j])
    assert differs > 0
    # the dividends of every set that holds contact j without pcre j are exactly 0 (the fp32 butterfly of cf_dividends_from_rows)
    a = rows.numpy().astype(np.float32).copy()
    for k in range(6):
        for s in range(64):
            if s >> k & 1:
                a[:, s] = a[:, s] - a[:, s ^ 1 << k]
    for s in range(64):
        if any(s >> (3 + j) & 1 and not s >> j & 1 for j in range(3)):
            assert (a[:, s] == 0).all(), s
    assert (a[:, 0b001001] != 0).any()


def test_scale_one_an_equal_donor_and_a_dummy_slot_are_null_exactly(small):
    cfg, batch, P, _, _ = small
    drop, contact, _ = _players("contacts", 3)
    words = [7, 0, 1, 2, 4, 5]
    with torch.no_grad():
        plain = orc.forward(P, batch, cfg)
    one = oracle_contact_coalitions(P, batch, words, drop, contact, 1.0, None, cfg)
    own = oracle_contact_coalitions(P, batch, words, drop, contact, 0.0, batch["interaction_freq"].clone(), cfg)
    zero = oracle_contact_coalitions(P, batch, words, drop, contact, 0.0, None, cfg)
    for c in range(len(words)):
        assert torch.equal(one[:, c], plain) and torch.equal(own[:, c], plain), c
    assert torch.equal(zero[:, 0], plain) and not torch.equal(zero[:3, 1], plain[:3])
    # gene 4 has no pCRE, gene 3 only slot 0: the other contacts are null players
    assert all(torch.equal(zero[4, c], plain[4]) for c in range(len(words)))
    assert torch.equal(zero[3, words.index(5)], zero[3, words.index(1)]) and torch.equal(zero[3, words.index(4)], zero[3, words.index(0)])


def test_fp64_shapley_values_of_the_oracle_table_are_efficient(small):
    cfg, batch, P, (drop, contact, names), rows = small
    phi, _ = shapley_fp64(rows.numpy())
    v = rows.numpy().astype(np.float64)
    gap = np.abs(phi.sum(1) - (v[:, 63] - v[:, 0])).max()
    print("joint game, i_max 3: efficiency gap of the fp64 Shapley values %.3e" % gap)
    assert gap < 1e-12
    dummy = torch.stack([m[:, 0, 0, 1:] for m in batch["interaction_masks"].values()]).all(0).numpy()
    for b in range(5):
        for j in range(3):
            if dummy[b, j]:
                assert (phi[b, j] == 0).all() and (phi[b, 3 + j] == 0).all(), (b, j)
    assert (np.abs(phi[:3]) > 1e-6).all()      # genes without dummies: chromatin state and contact both carry weight


def test_header_struct_and_bindings_agree():
    from chromoformer_amd import _lib
    hdr = " ".join(open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read().split())
    assert ("typedef struct cf_contact_opts { int n_players; /* 1..16 */ const uint32_t* player_drop;" in hdr)
    for name in ("cf_contact_coalitions", "cf_contact_shapley", "cf_contact_epistasis", "cf_contact_shapley_interactions"):
        assert "int %s(cf_handle* h, const cf_batch* batch, const cf_contact_opts* opts," % name in hdr and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    assert [f[0] for f in _lib.cf_contact_opts._fields_] == ["n_players", "player_drop", "player_contact", "scale", "donor_freq"]
    assert C.sizeof(_lib.cf_contact_opts) == 40 and _lib.cf_contact_opts.donor_freq.offset == 32 and _lib.cf_contact_opts.scale.offset == 24
    assert _lib.lib().cf_abi_version() == 1


CLI_MISUSE = [
    (["--contact-players", "all"], "--contact-players needs"),
    (["--contact-scale", "2"], "--contact-scale needs"),
    (["--contact-donor-marks", "donor"], "--contact-donor-marks needs --contact-donor-shapley-out"),
    (["--contact-donor-shapley-out", "x.npz"], "--contact-donor-shapley-out needs --donor-npy-dir"),
    (["--contact-donor-shapley-out", "x.npz", "--donor-npy-dir", "d", "--contact-scale", "0.5"], "the donor rule has no scale"),
    (["--contact-shapley-out", "x.npz", "--contact-scale", "nan"], "--contact-scale must be a finite factor"),
    (["--contact-shapley-out", "x.npz", "--contact-players", "cells"], "invalid choice"),
    (["--contact-interactions-out", "x.npy", "--contact-players", "all"], "at least 2 players"),
    (["--contact-shapley-out", "x.npz", "--contact-donor-marks", "donor"], "--contact-donor-marks needs"),
]


@pytest.mark.parametrize("extra, needle", CLI_MISUSE, ids=[" ".join(a for a in e if a.startswith("--")) for e, _ in CLI_MISUSE])
def test_predict_refuses_misused_contact_options(extra, needle, capsys):
    from chromoformer_amd import predict
    with pytest.raises(SystemExit) as e:
        predict.main(["-m", "meta.csv", "-d", "npy", "-o", "out.csv"] + extra)
    assert e.value.code == 2
    assert needle in capsys.readouterr().err
