"""The oracle's attention maps: the softmax of every attention call of orc.forward (orc._attend patched to record it), sliced to the
rows the model consumes -- the layout of ChromoformerBase.attention_maps.  Used by the attention-map tests and by
tests/golden/make_attention_map_goldens.py (which applies the same slicing to the reference's recorded att_prob)."""
import torch
import torch.nn.functional as F

from oracle import chromoformer_oracle as orc


def slice_maps(probs, B, cfg):
    """Softmax results in call order (Embedding layers per binsize, Pairwise layers per binsize, Regulation layers per binsize:
    net.py:341-373, the oracle's forward) -> {"embed.<b>": [B, nh, L] (centre query row), "pairwise_interaction.<b>":
    [B, n_layers, i_max, nh, L] (centre row per pCRE), "regulation.<b>": [B, n_layers, H, T] (row 0)}."""
    S = cfg["i_max"]
    n_e, n_p, n_r = cfg["embed"]["n_layers"], cfg["pairwise_interaction"]["n_layers"], cfg["regulation"]["n_layers"]
    it = iter(probs)
    out = {}
    for b in cfg["binsizes"]:
        ps = [next(it) for _ in range(n_e)]
        L = ps[0].shape[-1]
        out["embed.%d" % b] = ps[0][:, :, L // 2].reshape(B, -1, L)
    for b in cfg["binsizes"]:
        ps = [next(it) for _ in range(n_p)]
        L = ps[0].shape[-1]
        out["pairwise_interaction.%d" % b] = torch.stack([p[:, :, L // 2].reshape(B, S, -1, L) for p in ps], 1)
    for b in cfg["binsizes"]:
        ps = [next(it) for _ in range(n_r)]
        out["regulation.%d" % b] = torch.stack([p[:, :, 0] for p in ps], 1)
    assert next(it, None) is None
    return out


def oracle_maps(P, batch, cfg=None):
    """-> (logits, maps): maps as slice_maps plus "regulatory_embedding" (the fc_head input, net.py:375-378)."""
    c = orc._cfg(cfg)
    probs = []
    attend = orc._attend

    def recording(q, k, v, mask, extra=None):
        score = torch.matmul(q, k.transpose(-1, -2)) / (q.shape[-1] ** 0.5)
        if extra is not None:
            score = score + extra
        if mask is not None:
            score = score.masked_fill(mask, -1e9)
        probs.append(F.softmax(score, dim=-1))
        return attend(q, k, v, mask, extra)

    orc._attend = recording
    try:
        with torch.no_grad():
            logits, st = orc.forward(P, batch, cfg, return_stages=True)
    finally:
        orc._attend = attend
    maps = slice_maps(probs, logits.shape[0], c)
    maps["regulatory_embedding"] = (torch.cat([st["regulation_row0.%d" % b] for b in c["binsizes"]], 1)
                                    + torch.cat([st["embed_tss.%d" % b][:, 0] for b in c["binsizes"]], 1))
    return logits, maps
