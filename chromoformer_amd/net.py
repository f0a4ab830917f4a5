"""ChromoformerClassifier / ChromoformerRegressor on the MI355X HIP path.

Host-side mirror of the reference model interface (/root/reference/chromoformer/net.py:
273-428): same constructor arguments, same six-argument ``forward``, same
``state_dict()`` keys / shapes / order, same seeded initial weights.  All arithmetic is
done by libchromoformer_hip.so (csrc/); torch supplies device memory, streams and the
autograd hook only.  There is no PyTorch fallback: without the library or without a GPU
the model raises.

Two ways to train:
  * drop-in: ``out = model(...); loss = criterion(out, y); loss.backward()`` then a torch
    optimiser over ``model.parameters()`` (what the reference's train.py does);
  * fused:   ``model.train_step(batch, labels, lr)`` -- forward, loss, backward, optional
    gradient all-reduce and AdamW entirely inside the library (what bench.py and
    chromoformer_amd.train use).
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import _lib

_DEFAULT_EMBED = {"n_layers": 1, "n_heads": 2, "d_model": 128, "d_ff": 128}
_DEFAULT_PAIR = {"n_layers": 2, "n_heads": 2, "d_model": 128, "d_ff": 256}
_DEFAULT_REG = {"n_layers": 6, "n_heads": 8, "d_model": 256, "d_ff": 256}


def _positional_table(n_pos, dim):
    """Sinusoid table added to the token embeddings (net.py:23-29), float32 on the host."""
    pe = torch.zeros(n_pos, dim)
    pos = torch.arange(0, n_pos, 1).unsqueeze(1)
    k = torch.exp(-np.log(10000) * torch.arange(0, dim, 2) / dim)
    pe[:, 0::2] = torch.sin(pos * k)
    pe[:, 1::2] = torch.cos(pos * k)
    return pe.contiguous()


def _init_tensor(shape, fan_in, kind):
    """Default nn.Linear / nn.LayerNorm initialisers (same RNG draws as torch's)."""
    if kind == "ones":
        return torch.ones(shape)
    if kind == "zeros":
        return torch.zeros(shape)
    if kind == "weight":
        bound = math.sqrt(3.0) * math.sqrt(2.0 / (1 + math.sqrt(5) ** 2)) / math.sqrt(fan_in)  # kaiming_uniform_(a=sqrt(5))
    else:
        bound = 1.0 / math.sqrt(fan_in)
    return torch.empty(shape).uniform_(-bound, bound)


def _init_kind(name, shape):
    leaf = name.rsplit(".", 2)[-2:]
    if leaf[-1] == "gamma_f":
        return "ones", 0
    if leaf[0] == "ln":
        return ("ones", 0) if leaf[1] == "weight" else ("zeros", 0)
    if leaf[1] == "weight":
        return "weight", shape[1]
    return "bias", None  # fan_in resolved from the sibling weight


TRUNK_PREFIXES = ("embed.", "pairwise_interaction.")
FREEZE_GRANULARITY = ("freezing is supported for the whole trunk only -- every embed.* and pairwise_interaction.* tensor of every resolution "
                      "(CF_BUCKET_PE) frozen, every regulation.* and fc_head.* tensor (CF_BUCKET_REG) trainable -- not for single resolutions, "
                      "modules or layers")


def is_trunk_name(name):
    """Does a state_dict key (current naming) belong to the trunk, the Embedding + Pairwise modules?"""
    return name.startswith(TRUNK_PREFIXES)


def split_layout(table):
    """The frozen / stepped partition of a parameter table under a frozen trunk -> (trunk, top, never): names of the trainable trunk
    tensors (CF_BUCKET_PE), of the trainable Regulation + head tensors (CF_BUCKET_REG), and of the tensors no step ever writes."""
    trunk = [e["name"] for e in table if e["trainable"] and is_trunk_name(e["name"])]
    top = [e["name"] for e in table if e["trainable"] and not is_trunk_name(e["name"])]
    never = [e["name"] for e in table if not e["trainable"]]
    return trunk, top, never


class _BackwardHook(torch.autograd.Function):
    """Lets ``loss.backward()`` of the caller drive cf_backward_from(), or cf_backward_from_inputs() when one of the float inputs
    (the device float32 copies _pack made of them: promoter_feats[b] per resolution, pcre_feats[b] per resolution, interaction_freq)
    requires a gradient -- autograd carries it back through the .to() to the caller's tensor."""

    @staticmethod
    def forward(ctx, anchor, model, batch_struct, keep, *inputs):
        ctx.model, ctx.batch_struct, ctx.keep = model, batch_struct, keep
        ctx.shapes = [t.shape for t in inputs]
        ctx.maps_gen = model._maps_gen
        return model._run_forward(batch_struct, save=True)

    @staticmethod
    def backward(ctx, dlogits):
        m = ctx.model
        if ctx.maps_gen != m._maps_gen:
            raise RuntimeError("loss.backward(): %s() has run a forward pass since this output was computed and overwrote the "
                               "activations its backward pass needs; call model(...) again before backward()" % m._maps_by)
        dl = dlogits.contiguous().float()
        st = torch.cuda.current_stream(m._device).cuda_stream
        needs = ctx.needs_input_grad[4:]
        grads = [None] * len(needs)
        frozen = m._trunk_frozen()      # (raises for a freeze the library has no step for)
        if frozen and not any(needs):
            # every Embedding / Pairwise parameter has requires_grad == False: head + Regulation backward and their bucket's reductions only
            _lib.check(_lib.lib().cf_backward_from_top(m._handle, C.byref(ctx.batch_struct), dl.data_ptr(), st), "cf_backward_from_top")
        elif not any(needs):
            _lib.check(_lib.lib().cf_backward_from(m._handle, C.byref(ctx.batch_struct), dl.data_ptr(), st), "cf_backward_from")
        else:
            nres = (len(needs) - 1) // 2
            want = _lib.cf_input_grads()
            for i, need in enumerate(needs):
                if not need:
                    continue
                g = torch.empty(ctx.shapes[i], device=m._device, dtype=torch.float32)   # (written in full by the library)
                grads[i] = g
                if i < nres:
                    want.promoter_feats[i] = g.data_ptr()
                elif i < 2 * nres:
                    want.pcre_feats[i - nres] = g.data_ptr()
                else:
                    want.interaction_freq = g.data_ptr()
            _lib.check(_lib.lib().cf_backward_from_inputs(m._handle, C.byref(ctx.batch_struct), dl.data_ptr(), C.byref(want), st),
                       "cf_backward_from_inputs")
        m._publish_grads(top_only=frozen)
        m._grads_top = m._top_range() if frozen else None      # what active_grads() may hand out after this backward
        return (torch.zeros_like(m._anchor), None, None, None, *grads)


class ChromoformerBase(nn.Module):
    n_out = 2

    def __init__(self, n_feats=7, d_emb=128, d_head=128, embed_kws=None, pairwise_interaction_kws=None,
                 regulation_kws=None, binsizes=(2000, 500, 100), seed=42, i_max=8, w_max=40000, max_batch=64):
        super().__init__()
        torch.manual_seed(seed)
        embed = dict(_DEFAULT_EMBED if embed_kws is None else embed_kws)
        pair = dict(_DEFAULT_PAIR if pairwise_interaction_kws is None else pairwise_interaction_kws)
        reg = dict(_DEFAULT_REG if regulation_kws is None else regulation_kws)
        embed["d_model"] = d_emb                      # net.py:305
        self.binsizes = [int(b) for b in binsizes]    # accepts the CLI's strings (train.py:33)
        self.n_feats, self.d_emb, self.d_head = n_feats, d_emb, d_head
        self.i_max, self.w_max = i_max, w_max
        self.n_bins = [w_max // b for b in self.binsizes]
        self._kws = (embed, pair, reg)
        self._max_batch = max_batch
        self._maps_gen = 0          # bumped by attention_maps() / pcre_ablation() / pcre_coalitions() / pcre_shapley() / pcre_shapley_interactions() / pcre_epistasis() / integrated_gradients() / perturbation_scan() / perturbation_scan_regions() / perturbation_scan_fine() / trunk_outputs(): a pending backward of an earlier forward refuses to run
        self._maps_by = None        # ... naming the last of them
        self._handle = None
        self._device = None
        self._cfg = _lib.make_config(n_feats, d_emb, d_head, self.n_out, self.binsizes, self.n_bins, i_max, embed, pair, reg,
                                     max_batch)
        self._layout, self._table = _lib.param_layout(self._cfg)
        self._step = 0
        # seeded initial values, drawn in the reference's construction order (= state_dict order);
        # the regressor draws the 2-way head first and then a fresh 1-way head (net.py:411-428)
        draws = OrderedDict()
        entries = list(self._table)
        if self.n_out == 1:
            cfg2 = _lib.make_config(n_feats, d_emb, d_head, 2, self.binsizes, self.n_bins, i_max, embed, pair, reg, max_batch)
            entries = entries[:-4] + _lib.param_layout(cfg2)[1][-4:] + entries[-4:]
        fan = None
        for i, e in enumerate(entries):
            kind, fan_in = _init_kind(e["name"], e["shape"])
            if kind == "weight":
                fan = fan_in
            t = _init_tensor(e["shape"], fan if kind == "bias" else fan_in, kind)
            draws[e["name"]] = t          # later (regressor head) draws overwrite the earlier ones
        for e in self._table:
            self._register(e["name"], nn.Parameter(draws[e["name"]]))

    # ----------------------------------------------------------------- module plumbing
    def _register(self, dotted, param):
        mod = self
        parts = dotted.split(".")
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, nn.Module())
            mod = mod._modules[p]
        mod.register_parameter(parts[-1], param)

    def _named(self):
        return OrderedDict(self.named_parameters())

    def cuda(self, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: chromoformer_amd has no CPU fallback (use the oracle/ only for checking)")
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else
                           (device if isinstance(device, int) else torch.device(device).index or 0))
        return self._materialize(dev)

    def to(self, *args, **kwargs):
        dev = None
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, (str, torch.device)) and torch.device(a).type == "cuda":
                dev = torch.device(a)
        if dev is None:
            raise RuntimeError("chromoformer_amd runs on an MI355X only; .to() accepts a cuda device")
        return self.cuda(dev.index)

    def _materialize(self, dev):
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: chromoformer_amd has no CPU fallback (use the oracle/ only for checking)")
        named = self._named()
        lay = self._layout
        with torch.cuda.device(dev):
            flat = torch.zeros(lay.n_total, device=dev)
            for e in self._table:
                flat[e["offset"]:e["offset"] + e["numel"]].copy_(named[e["name"]].detach().reshape(-1))
            self._flat = flat
            self._gflat = torch.zeros(lay.n_total, device=dev)
            self._mflat = torch.zeros(lay.n_total, device=dev)
            self._vflat = torch.zeros(lay.n_total, device=dev)
            self._anchor = torch.zeros(1, device=dev, requires_grad=True)
            self._loss_buf = torch.zeros(1, device=dev)
            for e in self._table:
                named[e["name"]].data = flat[e["offset"]:e["offset"] + e["numel"]].view(e["shape"])
            if self._handle is not None:
                _lib.lib().cf_destroy(self._handle)
            pes = [_positional_table(n, self.d_emb).numpy() for n in self.n_bins]
            ptrs = (C.c_void_p * len(pes))(*[p.ctypes.data for p in pes])
            h = C.c_void_p()
            _lib.check(_lib.lib().cf_create(C.byref(self._cfg), ptrs, C.byref(h)), "cf_create")
            self._handle = h
            _lib.check(_lib.lib().cf_bind(h, flat.data_ptr(), self._gflat.data_ptr(), self._mflat.data_ptr(),
                                          self._vflat.data_ptr()), "cf_bind")
        self._device = dev
        return self

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().cf_destroy(self._handle)
        except Exception:
            pass

    def _publish_grads(self, top_only=False):
        named = self._named()
        for e in self._table:
            if e["trainable"] and not (top_only and is_trunk_name(e["name"])):
                named[e["name"]].grad = self._gflat[e["offset"]:e["offset"] + e["numel"]].view(e["shape"])

    def _trunk_frozen(self):
        """Have the trunk's parameters been frozen with requires_grad_(False)?  -> False (none frozen: the full backward) or True (EVERY
        Embedding and Pairwise tensor frozen, every Regulation / fc_head tensor trainable).  Anything else raises: the library steps the
        two ranges of the parameter layout whole.  (Runs in front of every loss.backward(): one pass over a cached list of the trainable
        parameters; the names are only looked at once something is frozen.)"""
        if getattr(self, "_freeze_list", None) is None:
            named = self._named()
            self._freeze_list = [(e["name"], named[e["name"]], is_trunk_name(e["name"])) for e in self._table if e["trainable"]]
        if all(p.requires_grad for _, p, _ in self._freeze_list):
            return False
        off = [n for n, p, _ in self._freeze_list if not p.requires_grad]
        top = [n for n, p, trunk in self._freeze_list if not trunk and not p.requires_grad]
        if top:
            raise RuntimeError("loss.backward(): parameter '%s' has requires_grad == False; %s" % (top[0], FREEZE_GRANULARITY))
        on = [n for n, p, trunk in self._freeze_list if trunk and p.requires_grad]
        if on:
            raise RuntimeError("loss.backward(): parameter '%s' has requires_grad == True while '%s' is frozen; %s" % (on[0], off[0], FREEZE_GRANULARITY))
        return True

    def _top_range(self):
        """The Regulation + head range (CF_BUCKET_REG) of the flat gradient buffer, from the parameter table."""
        lo = min(e["offset"] for e in self._table if e["trainable"] and not is_trunk_name(e["name"]))
        return self._gflat[lo: self._layout.n_active]

    def freeze_trunk(self, frozen=True):
        """requires_grad_(not frozen) on every Embedding and Pairwise parameter (the trunk); returns self."""
        for n, p in self._named().items():
            if is_trunk_name(n):
                p.requires_grad_(not frozen)
                if frozen:
                    p.grad = None
        return self

    def load_state_dict(self, state_dict, strict=True):
        out = super().load_state_dict(state_dict, strict=strict)   # copy_ into the flat-buffer views
        return out

    # ----------------------------------------------------------------- batches
    def _rows(self, mask, L, lead):
        """Centre-query-row pointer + stride of a pad mask: the reference's [.., 1, L, L] bool
        tensor (zero copy) or a compact [.., L] row array."""
        m = mask
        if m.dtype != torch.bool and m.dtype != torch.uint8:
            raise TypeError("pad masks must be bool / uint8")
        if not m.is_cuda:
            m = m.to(self._device)
        m = m.contiguous()
        if m.dim() >= 2 and m.shape[-1] == L and m.shape[-2] == L and m.numel() == lead * L * L:
            return m, m.data_ptr() + (L // 2) * L, L * L
        if m.numel() == lead * L:
            return m, m.data_ptr(), L
        raise ValueError("unexpected pad-mask shape %s" % (tuple(mask.shape),))

    def _pack(self, promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq, inputs=None):
        """inputs: an optional list that receives the device float32 copies of the float inputs, in the order promoter_feats per
        resolution, pcre_feats per resolution, interaction_freq (forward hands them to autograd)."""
        if self._handle is None:
            raise RuntimeError("call .cuda() first: the Chromoformer HIP path needs device buffers")
        bs = _lib.cf_batch()
        keep = []
        S, T = self.i_max, self.i_max + 1
        B = None
        pfs, cfs = [], []

        def dev_f32(t):
            t = t.to(self._device, torch.float32).contiguous()
            keep.append(t)
            return t

        for r, b in enumerate(self.binsizes):
            L = self.n_bins[r]
            pf, cf = dev_f32(promoter_feats[b]), dev_f32(pcre_feats[b])
            B = pf.shape[0] if B is None else B
            if pf.numel() != B * L * self.n_feats or cf.numel() != B * S * L * self.n_feats:
                raise ValueError("feature shapes do not match the configuration at binsize %d" % b)
            bs.promoter_feats[r], bs.pcre_feats[r] = pf.data_ptr(), cf.data_ptr()
            if inputs is not None:
                pfs.append(pf)
                cfs.append(cf)
            m, ptr, stride = self._rows(promoter_pad_masks[b], L, B)
            keep.append(m)
            bs.promoter_mask_row[r], bs.promoter_mask_stride[r] = ptr, stride
            m, ptr, stride = self._rows(pcre_pad_masks[b], L, B * S)
            keep.append(m)
            bs.pcre_mask_row[r], bs.pcre_mask_stride[r] = ptr, stride
            im = interaction_masks[b].to(self._device).contiguous()
            if im.numel() != B * T * T:
                raise ValueError("interaction mask shape mismatch at binsize %d" % b)
            keep.append(im)
            bs.interaction_mask[r] = im.data_ptr()
        fr = dev_f32(interaction_freq)
        if fr.numel() != B * T * T:
            raise ValueError("interaction_freq shape mismatch")
        bs.interaction_freq = fr.data_ptr()
        bs.B = B
        if B > self._max_batch:
            raise ValueError("batch of %d genes exceeds max_batch=%d given at construction" % (B, self._max_batch))
        if inputs is not None:
            inputs.extend(pfs + cfs + [fr])
        return bs, keep

    def pack_batch(self, d):
        """Pack a reference-layout batch dict (data.py:205-212) once, for repeated steps."""
        return self._pack(d["promoter_feats"], d["promoter_pad_masks"], d["pcre_feats"], d["pcre_pad_masks"],
                          d["interaction_masks"], d["interaction_freq"])

    # ----------------------------------------------------------------- forward / backward
    # ----------------------------------------------------------------- tiled weight copies kept fresh by the fused optimiser (cf_keep_tiled)
    def keep_tiled(self, on=True):
        """The fused optimiser writes the tiled copies of the Embedding + Pairwise weights it steps, forward passes stop re-tiling them
        (Trainer: no launch in front of a training step).  Whatever else writes parameters THROUGH TORCH -- load_state_dict, an optimiser,
        an in-place op on a parameter -- is noticed by the version counters (_sync_tiled, in front of every forward pass); an edit through
        `.data` or a raw pointer is not: call params_changed() after it.  Returns whether the library offers the mode for this model."""
        ok = _lib.lib().cf_keep_tiled(self._handle, 1 if on else 0) == 0
        self._keep_tiled = bool(on) and ok
        self._pver = None
        return self._keep_tiled

    def params_changed(self):
        if self._handle is not None:
            _lib.check(_lib.lib().cf_params_changed(self._handle), "cf_params_changed")
        self._pver = None

    def _sync_tiled(self, st):
        """In front of every forward pass of a model in keep_tiled mode: have parameters been written through torch since the library last
        saw them?  (sum of the version counters of the ~370 parameters: ~20 us of host time.)  If so the tiled copies are rebuilt at once, on
        the stream the pass will run on -- also in front of a hipGraph that was captured without the re-tiling."""
        if not getattr(self, "_keep_tiled", False):
            return
        if getattr(self, "_plist", None) is None:
            self._plist = [p for _, p in self.named_parameters()]
        ver = sum(p._version for p in self._plist)
        if ver != self._pver:
            _lib.check(_lib.lib().cf_params_changed(self._handle), "cf_params_changed")
            _lib.check(_lib.lib().cf_retile_early(self._handle, st), "cf_retile_early")
            self._pver = ver

    def _run_forward(self, bs, save):
        """save: False / 0 = inference, True / 1 = keep activations, 2 = as 1 with the head left to the cf_backward that follows."""
        out = torch.empty(bs.B, self.n_out, device=self._device)
        st = torch.cuda.current_stream(self._device).cuda_stream
        self._sync_tiled(st)
        _lib.check(_lib.lib().cf_forward(self._handle, C.byref(bs), out.data_ptr(), int(save), st), "cf_forward")
        return out

    def forward(self, promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq):
        if not torch.is_grad_enabled():
            bs, keep = self._pack(promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq)
            return self._run_forward(bs, save=False)
        inputs = []
        bs, keep = self._pack(promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq,
                              inputs=inputs)
        # the float inputs go in as arguments: a gradient requested for any of them is computed by the library (saliency maps)
        return _BackwardHook.apply(self._anchor, self, bs, keep, *inputs)

    MAP_KEYS = ("embed", "pairwise_interaction", "regulation", "regulatory_embedding")

    def _attrib_call(self, who, args):
        """What the attribution methods share -> (batch struct, keep-alive, book).  `args`: the six tensors of forward(), or a packed
        batch (an engine.Slot, a pack_batch result or a batch struct) with None after it.  book() -> stream, called directly in front
        of the library call, once the arguments are accepted: it brings the tiled weights up to date on the stream and books the call
        as `who` (a pending backward of an earlier forward then refuses to run)."""
        if args[1] is None:
            p = args[0]
            bs, keep = (p if isinstance(p, _lib.cf_batch) else p.struct if hasattr(p, "struct") else p[0]), p
        else:
            bs, keep = self._pack(*args)
        if self._handle is None:
            raise RuntimeError("call .cuda() first: the Chromoformer HIP path needs device buffers")

        def book():
            st = torch.cuda.current_stream(self._device).cuda_stream
            self._sync_tiled(st)
            self._maps_gen += 1
            self._maps_by = who
            return st

        return bs, keep, book

    @torch.no_grad()
    def attention_maps(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                       interaction_freq=None, which=MAP_KEYS):
        """Logits and what a user of the reference reads off its attention modules (modules.py:73, 184) and fc_head input, from one
        forward pass (cf_attention_maps) -> (logits [B, n_out], maps), tensors on the model's device.  Per binsize b, L = n_bins[b],
        T = i_max + 1:

          maps["embed"][b]                 [B, embed.n_heads, L]                       centre query's softmax row of the Embedding layer
          maps["pairwise_interaction"][b]  [B, pw.n_layers, i_max, pw.n_heads, L]     promoter centre row over each pCRE's bins, per layer
          maps["regulation"][b]            [B, reg.n_layers, reg.n_heads, T]           row 0 (promoter token) over [promoter, pCRE slots]
          maps["regulatory_embedding"]     [B, 3 * d_emb]                              cat(x_out[b][:, 0]) + cat(x_in[b][:, 0])

        Masked keys are 0, fully masked rows (dummy pCRE slots) uniform, as with the reference.  `which` selects the outputs (the others
        are not copied).  The first argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.
        The pass overwrites the activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        bs, _keep, book = self._attrib_call("attention_maps", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        which = (which,) if isinstance(which, str) else tuple(which)
        bad = [k for k in which if k not in self.MAP_KEYS]
        if bad:
            raise ValueError("attention_maps: unknown output(s) %s; choose from %s" % (bad, self.MAP_KEYS))
        B, S, T, dev = bs.B, self.i_max, self.i_max + 1, self._device
        embed, pair, reg = self._kws
        want = _lib.cf_attn_maps()
        maps = {k: {} for k in which if k != "regulatory_embedding"}
        for r, b in enumerate(self.binsizes):
            L = self.n_bins[r]
            for key, field, shape in (("embed", "embed", (B, embed["n_heads"], L)),
                                      ("pairwise_interaction", "pairwise", (B, pair["n_layers"], S, pair["n_heads"], L)),
                                      ("regulation", "regulation", (B, reg["n_layers"], reg["n_heads"], T))):
                if key in maps:
                    t = maps[key][b] = torch.empty(shape, device=dev)      # (written in full by the library)
                    getattr(want, field)[r] = t.data_ptr()
        if "regulatory_embedding" in which:
            maps["regulatory_embedding"] = t = torch.empty(B, len(self.binsizes) * self.d_emb, device=dev)
            want.embedding = t.data_ptr()
        logits = torch.empty(B, self.n_out, device=dev)
        st = book()
        _lib.check(_lib.lib().cf_attention_maps(self._handle, C.byref(bs), logits.data_ptr(), C.byref(want), st), "cf_attention_maps")
        return logits, maps

    @torch.no_grad()
    def pcre_ablation(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                      interaction_freq=None):
        """In-silico pCRE deletion (cf_pcre_ablation) -> logits [B, i_max + 2, n_out] on the model's device, no autograd graph:

          [:, 0]          the prediction (model(...) under no_grad, bit-equal)
          [:, 1 + j]      with pCRE slot j deleted: interaction_masks row and column j + 1 set at every resolution (= the slot made a
                          dataset dummy, data.py); a slot that is already a dummy gives [:, 0]
          [:, i_max + 1]  the promoter alone: rows and columns 1..i_max set

        The Embedding + Pairwise stage runs once, the Regulation stack and the head on the B * (i_max + 2) gene-variants.  The first
        argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.  The pass overwrites the
        activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        bs, _keep, book = self._attrib_call("pcre_ablation", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        logits = torch.empty(bs.B, self.i_max + 2, self.n_out, device=self._device)      # (written in full by the library)
        st = book()
        _lib.check(_lib.lib().cf_pcre_ablation(self._handle, C.byref(bs), logits.data_ptr(), st), "cf_pcre_ablation")
        return logits

    @torch.no_grad()
    def pcre_coalitions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                        interaction_freq=None, keep=None):
        """The prediction under pCRE coalitions (cf_pcre_coalitions) -> logits [B, n_coal, n_out] on the model's device, no autograd
        graph.  `keep`: a sequence / array of ints, bit j set = pCRE slot j kept, or a bool array [n_coal, i_max].  Column c is the
        inference forward with interaction_masks row and column j + 1 set, at every resolution, for every slot j that keep[c] drops
        (model(...) under no_grad on those masks, bit-equal): 2^i_max - 1 is the prediction, 0 the promoter alone; a bit of a slot
        that is already a dummy changes nothing; a bit >= i_max raises ValueError.  The Embedding + Pairwise stage runs once, the
        Regulation stack and the head on the B * n_coal rows.  The first argument may also be a packed batch (an engine.Slot or a
        pack_batch result), with nothing after it.  The pass overwrites the activations a grad-enabled model(...) keeps for its
        backward: such a pending backward() raises."""
        from .attribution import coalition_words
        if keep is None:
            raise ValueError("pcre_coalitions: keep is required: the coalition words (bit j set: pCRE slot j kept)")
        words = coalition_words(keep, self.i_max, "pcre_coalitions")
        bs, _keep, book = self._attrib_call("pcre_coalitions", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        logits = torch.empty(bs.B, len(words), self.n_out, device=self._device)      # (written in full by the library)
        st = book()
        _lib.check(_lib.lib().cf_pcre_coalitions(self._handle, C.byref(bs), words.ctypes.data, len(words), logits.data_ptr(), st),
                   "cf_pcre_coalitions")
        return logits

    @torch.no_grad()
    def pcre_shapley(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                     interaction_freq=None, return_coalitions=False):
        """Exact Shapley values of the pCRE slots (cf_pcre_shapley) -> (phi, info), tensors on the model's device, no autograd graph:

          phi                    [B, i_max, n_out]: slot j's average marginal contribution to each logit over all orders of adding
                                 the pCREs to the promoter; exactly 0 for a dummy slot
          info["logits"]         [B, n_out]: the prediction (all pCREs kept; model(...) under no_grad, bit-equal)
          info["promoter_only"]  [B, n_out]: the promoter alone
          info["delta"]          [B, n_out]: phi.sum(1) - (logits - promoter_only), the efficiency gap (rounding only)
          info["coalitions"]     [B, 2^i_max, n_out], with return_coalitions: the logits of every coalition, word m at column m

        All 2^i_max coalitions run from one trunk pass (pcre_coalitions); the values are in logit space, where efficiency holds.
        The first argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.  The pass
        overwrites the activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        bs, _keep, book = self._attrib_call("pcre_shapley", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        n = 1 << self.i_max
        rows = torch.empty(bs.B, n, self.n_out, device=self._device)      # (both written in full by the library)
        phi = torch.empty(bs.B, self.i_max, self.n_out, device=self._device)
        st = book()
        _lib.check(_lib.lib().cf_pcre_shapley(self._handle, C.byref(bs), phi.data_ptr(), rows.data_ptr(), st), "cf_pcre_shapley")
        info = {"logits": rows[:, n - 1].clone(), "promoter_only": rows[:, 0].clone()}
        info["delta"] = phi.sum(1) - (info["logits"] - info["promoter_only"])
        if return_coalitions:
            info["coalitions"] = rows
        return phi, info

    @torch.no_grad()
    def pcre_shapley_interactions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                  interaction_freq=None, index="sii", return_coalitions=False):
        """Pairwise Shapley interaction indices of the pCRE slots (cf_pcre_shapley_interactions) -> (inter, info), tensors on the
        model's device, no autograd graph.  P = i_max (at least 2); the 2^i_max coalitions run once, as in pcre_shapley:

          inter               [B, P, P, n_out], exactly symmetric.  Off the diagonal, with S over the coalitions that hold neither player,
                              I_ij = sum_S w(|S|) ((v(S + i + j) - v(S + j)) - (v(S + i) - v(S))): how much i's marginal contribution
                              changes with j present, averaged over every context -- negative for redundant players, positive for
                              cooperating ones, also where a third player hides the effect from the full-coalition *_epistasis.  index "sii"
                              (Shapley interaction index): w(s) = s! (P - s - 2)! / (P - 1)!, the diagonal is phi.  index "sti"
                              (Shapley-Taylor, order 2): w(s) = (2 / P) / C(P - 1, s), the diagonal is v({i}) - v(nobody), and the
                              diagonal plus the upper triangle sums to logits - promoter_only.  A null player's row and column are exactly 0
          info["phi"]         [B, P, n_out]: the Shapley values of pcre_shapley on the same rows, bit for bit
          info["logits"]      [B, n_out]: the prediction;  info["promoter_only"]  [B, n_out]: every player absent
          info["index"]       the index name;  info["delta"]  [B, n_out], "sti" only: the efficiency gap (rounding only)
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        SHAP's interaction values follow from the sii result: Phi_ij = I_ij / 2 off the diagonal and Phi_ii = phi_i - sum_{j != i} I_ij / 2.
        The packed forms of the first argument and the effect on a pending backward() are those of pcre_shapley."""
        from .attribution import interaction_index
        code = interaction_index(index, "pcre_shapley_interactions")
        bs, _keep, book = self._attrib_call("pcre_shapley_interactions", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        S = self.i_max
        rows = torch.empty(bs.B, 1 << S, self.n_out, device=self._device)      # (all three written in full by the library)
        inter = torch.empty(bs.B, S, S, self.n_out, device=self._device)
        phi = torch.empty(bs.B, S, self.n_out, device=self._device)
        st = book()
        _lib.check(_lib.lib().cf_pcre_shapley_interactions(self._handle, C.byref(bs), code, inter.data_ptr(), phi.data_ptr(), rows.data_ptr(), st),
                   "cf_pcre_shapley_interactions")
        return inter, self._interactions_info(inter, phi, rows, index, "promoter_only", None, return_coalitions)

    @torch.no_grad()
    def shapley_interactions(self, coalitions, index="sii"):
        """Pairwise Shapley interaction indices from a kept coalition table (cf_shapley_interactions_from_rows) -> inter
        [B, P, P, n_out] on the model's device: `coalitions` is info["coalitions"] of any exact *_shapley call, [B, 2^P, n_out] with
        word m at column m, 2 <= P <= 16 (a float32 tensor; moved to the model's device and made contiguous if it is not).  The bits
        are those of the *_shapley_interactions call on the same table (index as there); no forward runs and a pending backward() is
        left alone.
        SHAP's interaction values follow from the sii result: Phi_ij = I_ij / 2 off the diagonal and Phi_ii = phi_i - sum_{j != i} I_ij / 2."""
        from .attribution import interaction_index
        code = interaction_index(index, "shapley_interactions")
        if not torch.is_tensor(coalitions) or coalitions.dim() != 3 or coalitions.dtype != torch.float32:
            raise ValueError("shapley_interactions: coalitions must be a float32 tensor [B, 2^P, n_out]")
        B, n, n_out = coalitions.shape
        P = n.bit_length() - 1
        if B < 1 or n != 1 << P or not 2 <= P <= 16 or n_out != self.n_out:
            raise ValueError("shapley_interactions: coalitions has shape %s; expected [B >= 1, 2^P with P in 2..16, n_out = %d]"
                             % (tuple(coalitions.shape), self.n_out))
        if self._handle is None:
            raise RuntimeError("shapley_interactions: the model is not on a GPU (model.cuda() first); there is no CPU fallback")
        rows = coalitions.to(self._device).contiguous()
        inter = torch.empty(B, P, P, n_out, device=self._device)      # (written in full by the library)
        st = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(_lib.lib().cf_shapley_interactions_from_rows(self._handle, rows.data_ptr(), B, P, code, inter.data_ptr(), st),
                   "cf_shapley_interactions_from_rows")
        return inter

    def _table_check(self, who, what, table):
        """A [B, 2^P, n_out] float32 table on the model's device, contiguous -> (table, B, P)."""
        if not torch.is_tensor(table) or table.dim() != 3 or table.dtype != torch.float32:
            raise ValueError("%s: %s must be a float32 tensor [B, 2^P, n_out]" % (who, what))
        B, n, n_out = table.shape
        P = n.bit_length() - 1
        if B < 1 or n != 1 << P or not 1 <= P <= 16 or n_out != self.n_out:
            raise ValueError("%s: %s has shape %s; expected [B >= 1, 2^P with P in 1..16, n_out = %d]" % (who, what, tuple(table.shape), self.n_out))
        if self._handle is None:
            raise RuntimeError("%s: the model is not on a GPU (model.cuda() first); there is no CPU fallback" % who)
        return table.to(self._device).contiguous(), B, P

    @torch.no_grad()
    def shapley_dividends(self, coalitions, return_mass=False):
        """Harsanyi dividends (the Moebius transform) of a kept coalition table (cf_dividends_from_rows) -> div [B, 2^P, n_out] on the
        model's device, or (div, mass) with return_mass.  `coalitions` is info["coalitions"] of any exact *_shapley call, word m at
        column m, 1 <= P <= 16.  div[b, S] = sum over T <= S of (-1)^(|S| - |T|) v(T): what the players of S contribute TOGETHER beyond
        every smaller group of them; the dividends of all subsets of S add back up to v(S).  The fp32 result is the in-place
        butterfly (for k < P, for S with bit k: a[S] -= a[S ^ 1 << k]), bit for bit; the dividends of a set that holds a null player
        are exactly 0.  mass[b, S] = sum over T <= S of |v(T)| scales the rounding error (attribution.dividend_bound): a high-order
        dividend smaller than its bound is noise.  No forward runs and a pending backward() is left alone."""
        rows, B, P = self._table_check("shapley_dividends", "coalitions", coalitions)
        div = torch.empty_like(rows)      # (written in full by the library)
        mass = torch.empty_like(rows) if return_mass else None
        st = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(_lib.lib().cf_dividends_from_rows(self._handle, rows.data_ptr(), B, P, div.data_ptr(), mass.data_ptr() if return_mass else None, st),
                   "cf_dividends_from_rows")
        return (div, mass) if return_mass else div

    @torch.no_grad()
    def set_interactions(self, dividends, order=2, index="sii", sets=None):
        """An interaction index of sets of up to `order` players from the dividends (cf_set_interactions_from_dividends) -> (inter
        [B, n_sets, n_out] on the model's device, sets uint32 [n_sets]).  dividends: shapley_dividends' result; sets: words (bit p =
        player p), each with 1..order players; default attribution.interaction_sets(P, order), every such set by size and word.
        index "sii": the Shapley interaction index of any order (order 1 the Shapley values, order 2 the pairwise sii of
        shapley_interactions, within rounding); "sti": Shapley-Taylor of top order `order` -- sets below it carry their dividend's
        bits, and all sets together sum to logits - absent.  Weights: attribution.set_interaction_weights.  No forward runs."""
        from .attribution import interaction_index, interaction_sets
        who = "set_interactions"
        code = interaction_index(index, who)
        div, B, P = self._table_check(who, "dividends", dividends)
        order = int(order)
        if not 1 <= order <= P:
            raise ValueError("%s: order = %d outside 1..P = %d" % (who, order, P))
        if sets is None:
            words = interaction_sets(P, order)
        else:
            raw = np.asarray(sets.cpu() if hasattr(sets, "cpu") else sets)
            if raw.ndim != 1 or raw.size < 1 or raw.dtype.kind not in "iu" or raw.min() < 0 or raw.max() >= 1 << P:
                raise ValueError("%s: sets must be a non-empty 1-D integer array of words below 2^P = %d" % (who, 1 << P))
            words = np.ascontiguousarray(raw.astype(np.uint32))
        inter = torch.empty(B, len(words), self.n_out, device=self._device)      # (written in full by the library)
        st = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(_lib.lib().cf_set_interactions_from_dividends(self._handle, div.data_ptr(), B, P, words.ctypes.data, len(words), code, order,
                                                                 inter.data_ptr(), st), "cf_set_interactions_from_dividends")
        return inter, words

    def _dividends_info(self, phi, info, names):
        """(div, info) of a *_dividends call from its sibling's (phi, info with the coalitions)."""
        from .attribution import set_names
        div, mass = self.shapley_dividends(info["coalitions"], return_mass=True)
        info = dict(info, phi=phi, mass=mass, names=list(names))
        info["sets"] = set_names(np.arange(div.shape[1], dtype=np.uint32), names)
        return div, info

    @torch.no_grad()
    def pcre_dividends(self, *args, **kwargs):
        """pcre_shapley(..., return_coalitions=True) with the same arguments, then shapley_dividends on its table -> (div, info): div
        [B, 2^i_max, n_out], word m at column m; info is pcre_shapley's (logits, promoter_only, delta, coalitions) plus phi (its
        Shapley values, bit for bit), mass (shapley_dividends), names ("pcre0", ...) and sets (the 2^P set names by word, "" for the
        empty set).  A dummy slot is a null player: every set that holds it has dividend exactly 0."""
        phi, info = self.pcre_shapley(*args, **dict(kwargs, return_coalitions=True))
        return self._dividends_info(phi, info, ["pcre%d" % j for j in range(self.i_max)])

    @torch.no_grad()
    def mark_dividends(self, *args, **kwargs):
        """mark_shapley(..., return_coalitions=True) with the same arguments, then shapley_dividends -> (div, info) as pcre_dividends;
        info is mark_shapley's (logits, erased, players, delta, coalitions) plus phi, mass, names and sets."""
        phi, info = self.mark_shapley(*args, **dict(kwargs, return_coalitions=True))
        return self._dividends_info(phi, info, info["players"])

    @torch.no_grad()
    def mark_donor_dividends(self, *args, **kwargs):
        """mark_donor_shapley(..., return_coalitions=True) with the same arguments, then shapley_dividends -> (div, info) as
        mark_dividends; the absent key is "donor"."""
        phi, info = self.mark_donor_shapley(*args, **dict(kwargs, return_coalitions=True))
        return self._dividends_info(phi, info, info["players"])

    @torch.no_grad()
    def mark_window_dividends(self, *args, **kwargs):
        """mark_window_shapley(..., return_coalitions=True) with the same arguments (at most 16 window players), then
        shapley_dividends -> (div, info) as mark_dividends."""
        phi, info = self.mark_window_shapley(*args, **dict(kwargs, return_coalitions=True))
        return self._dividends_info(phi, info, info["players"])

    @torch.no_grad()
    def mark_fine_window_dividends(self, *args, **kwargs):
        """mark_fine_window_shapley(..., return_coalitions=True) with the same arguments (at most 16 fine window players), then
        shapley_dividends -> (div, info) as mark_dividends."""
        phi, info = self.mark_fine_window_shapley(*args, **dict(kwargs, return_coalitions=True))
        return self._dividends_info(phi, info, info["players"])

    @torch.no_grad()
    def pcre_epistasis(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                       interaction_freq=None):
        """Pair-deletion epistasis of the pCRE slots (cf_pcre_epistasis) -> (eps, info), tensors on the model's device, no autograd graph.
        With v(...) the logits after deleting the named slots from the full gene:

          eps[:, i, j]    [B, i_max, i_max, n_out]: ((v() - v(i)) - v(j)) + v(i, j) for i != j, exactly symmetric: 0 when the two
                          deletions add up, non-zero when the pCREs are redundant or cooperate; eps[:, i, i] = v() - v(i), the
                          leave-one-out effect; rows and columns of dummy slots are exactly 0
          info["logits"]  [B, n_out]: v(), the prediction;  info["single"]  [B, i_max, n_out]: v(i)

        The 1 + i_max + i_max (i_max - 1) / 2 rows (attribution.coalition_table("pairs", i_max)) run from one trunk pass.  The first
        argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.  The pass overwrites the
        activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        bs, _keep, book = self._attrib_call("pcre_epistasis", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        S = self.i_max
        rows = torch.empty(bs.B, 1 + S + S * (S - 1) // 2, self.n_out, device=self._device)      # (both written in full by the library)
        eps = torch.empty(bs.B, S, S, self.n_out, device=self._device)
        st = book()
        _lib.check(_lib.lib().cf_pcre_epistasis(self._handle, C.byref(bs), eps.data_ptr(), rows.data_ptr(), st), "cf_pcre_epistasis")
        return eps, {"logits": rows[:, 0].clone(), "single": rows[:, 1:1 + S].clone()}

    @torch.no_grad()
    def integrated_gradients(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                             interaction_freq=None, target=None, n_steps=50, method="gausslegendre", baselines=None,
                             inputs=("promoter_feats", "pcre_feats", "interaction_freq"), path="linear", donor=None):
        """Integrated gradients of logit column `target` (default: 1 for the classifier, 0 for the regressor) with respect to the float
        inputs named in `inputs` (cf_integrated_gradients) -> (attr, info), tensors on the model's device, no autograd graph:

          attr["promoter_feats"][b], attr["pcre_feats"][b], attr["interaction_freq"]   the caller's shapes (inputs not named: absent)
          info["logits"], info["baseline_logits"]   [B, n_out]: the forward of x and of the baseline
          info["delta"]                             [B]: sum of a gene's attributions - (logits - baseline_logits)[:, target]

        With nodes a_k and weights w_k of chromoformer_amd.attribution.ig_quadrature(method, n_steps): x_k = xb + a_k (x - xb),
        g_k = d(w_k logits[:, target]) / d x_k, attr = (x - xb) * (g_0 + g_1 + ... + g_{n-1}) -- what a hand-written loop of
        grad-enabled model(...) calls and backward()s gives, bit for bit.  `baselines`: None (zeros, the binned value of an empty
        signal) or a dict with some of the three keys ({binsize: tensor} for the features), each with a leading dimension of B or 1.
        Masks are never interpolated.  The first argument may also be a packed batch (an engine.Slot or a pack_batch result), with
        nothing after it.  Parameter gradients and optimiser state are left as they are; the pass overwrites the activations a
        grad-enabled model(...) keeps for its backward: such a pending backward() raises.

        path="signal" (cf_integrated_gradients_raw): the features are u = log(1 + m), m the mean of a bin of the raw signal, and the
        path is a * m from the empty signal -- straight in the raw signal, curved in the features: u_k = log1p(a_k expm1(u)),
        C = sum_k g_k / (1 + a_k m).  attr of the features is m * C, integrated gradients with respect to the bin means (still
        complete: delta as above), and info gains "coeff": {"promoter_feats": {b: ...}, "pcre_feats": {b: ...}} = (1 + m) * C, the dfeat
        that cf_bin_regions_multi_backward(times_input = 1) turns into per-sample attributions (attribution.raw_integrated_gradients).
        interaction_freq, if named, keeps its straight path and baseline.  `inputs` must name a feature input; a feature baseline
        raises ValueError (zero signal only); features must stay below ~80 (expm1 in fp32).

        path="signal" with donor=(donor_promoter_feats, donor_pcre_feats) (cf_integrated_gradients_raw_donor): the baseline is the same
        genes' binned signal in another cell type, in any form mark_donor_shapley's `donor` takes, and the path is the straight line
        xd + a (x - xd) between the two RAW signals: with m, md the bin means of the two, u_k = log1p(md + a_k (m - md)),
        C = sum_k g_k / (1 + md + a_k (m - md)), attr = (m - md) * C.  info["baseline_logits"] is the donor's features under the gene's
        masks and frequencies, info["cmean"] (in place of "coeff") = C per bin, which cf_bin_spread_difference spreads over the
        difference of the two raw signals.  An element with the same bits in both gets exactly 0; a donor of zeros gives the bits of
        the call without donor.  donor= with path="linear", or together with a feature baseline, raises ValueError."""
        from .attribution import INPUTS, ig_quadrature
        if path not in ("linear", "signal"):
            raise ValueError("integrated_gradients: path %r; choose 'linear' or 'signal'" % (path,))
        signal = path == "signal"
        if donor is not None:      # (before anything touches the device)
            if not signal:
                raise ValueError("integrated_gradients: donor= is the baseline of path='signal' (a path between two raw signals); "
                                 "path='linear' takes feature baselines in baselines=")
            given = [k for k in ("promoter_feats", "pcre_feats") if (baselines or {}).get(k) is not None]
            if given:
                raise ValueError("integrated_gradients: donor= and a baseline for %s: the donor is the feature baseline" % given)
            named = (inputs,) if isinstance(inputs, str) else tuple(inputs)
            if not set(named) & {"promoter_feats", "pcre_feats"}:
                raise ValueError("integrated_gradients: path='signal' needs promoter_feats or pcre_feats in inputs, got %s" % (named,))
        elif signal:
            named = (inputs,) if isinstance(inputs, str) else tuple(inputs)
            given = [k for k in ("promoter_feats", "pcre_feats") if (baselines or {}).get(k) is not None]
            if given:
                raise ValueError("integrated_gradients: path='signal' starts at the zero signal; a baseline for %s is not accepted" % given)
            if not set(named) & {"promoter_feats", "pcre_feats"}:
                raise ValueError("integrated_gradients: path='signal' needs promoter_feats or pcre_feats in inputs, got %s" % (named,))
        bs, _keep, book = self._attrib_call("integrated_gradients", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        shapes = None
        if promoter_pad_masks is not None:      # (given tensors: the attributions come back in the callers' shapes)
            shapes = {"promoter_feats": {b: promoter_feats[b].shape for b in self.binsizes},
                      "pcre_feats": {b: pcre_feats[b].shape for b in self.binsizes}, "interaction_freq": interaction_freq.shape}
        inputs = (inputs,) if isinstance(inputs, str) else tuple(inputs)
        bad = [k for k in inputs if k not in INPUTS]
        if bad or not inputs:
            raise ValueError("integrated_gradients: inputs %s; choose a non-empty subset of %s" % (bad or "()", INPUTS))
        target = (1 if self.n_out == 2 else 0) if target is None else int(target)
        alphas, weights = ig_quadrature(method, n_steps)
        B, S, T, F, dev = bs.B, self.i_max, self.i_max + 1, self.n_feats, self._device
        canon = {"promoter_feats": {b: (B, L, F) for b, L in zip(self.binsizes, self.n_bins)},
                 "pcre_feats": {b: (B, S, L, F) for b, L in zip(self.binsizes, self.n_bins)}, "interaction_freq": (B, T, T)}
        opts = _lib.cf_ig_opts()
        opts.n_steps, opts.target = len(alphas), target
        opts.interpolate = sum(bit for k, bit in zip(INPUTS, (_lib.IG_PROMOTER, _lib.IG_PCRE, _lib.IG_FREQ)) if k in inputs)
        opts.alphas, opts.weights = alphas.ctypes.data, weights.ctypes.data
        keep = []
        baselines = baselines or {}
        extra = [k for k in baselines if k not in INPUTS]
        if extra:
            raise ValueError("integrated_gradients: unknown baseline(s) %s; keys are %s" % (extra, INPUTS))
        unused = [k for k in baselines if baselines[k] is not None and k not in inputs]
        if unused:
            raise ValueError("integrated_gradients: baseline(s) given for %s, which are not in inputs=%s" % (unused, inputs))
        leads = set()
        for k in inputs:
            if baselines.get(k) is None:
                continue
            for t in (baselines[k].values() if isinstance(baselines[k], dict) else [baselines[k]]):
                leads.add(t.shape[0])
        if leads - {1, B}:
            raise ValueError("integrated_gradients: baselines need a leading dimension of B = %d or 1, got %s" % (B, sorted(leads)))
        bcast = leads == {1}

        def base(t, shape):
            n = 1 if bcast else B
            t = t.to(dev, torch.float32)
            if t.numel() != n * int(np.prod(shape[1:])):
                t = t.expand(B, *t.shape[1:]) if t.shape[0] == 1 else t
                if t.numel() != n * int(np.prod(shape[1:])):
                    raise ValueError("integrated_gradients: a baseline of %d elements does not match the input's shape %s" % (t.numel(), tuple(shape)))
            t = t.contiguous()
            keep.append(t)
            return t.data_ptr()

        for r, b in enumerate(self.binsizes):
            if "promoter_feats" in inputs and baselines.get("promoter_feats") is not None:
                opts.base_promoter_feats[r] = base(baselines["promoter_feats"][b], canon["promoter_feats"][b])
            if "pcre_feats" in inputs and baselines.get("pcre_feats") is not None:
                opts.base_pcre_feats[r] = base(baselines["pcre_feats"][b], canon["pcre_feats"][b])
        if "interaction_freq" in inputs and baselines.get("interaction_freq") is not None:
            opts.base_interaction_freq = base(baselines["interaction_freq"], canon["interaction_freq"])
        opts.base_broadcast = 1 if bcast else 0
        if donor is not None:
            if bcast:
                raise ValueError("integrated_gradients: donor= holds one row per gene; a broadcast baseline (leading dimension 1) cannot go with it")
            dn = _lib.cf_mark_donor_opts()
            keep.append(self._donor_feats("integrated_gradients", donor, B, dn))
            for r in range(len(self.binsizes)):
                if "promoter_feats" in inputs:
                    opts.base_promoter_feats[r] = dn.donor_promoter_feats[r]
                if "pcre_feats" in inputs:
                    opts.base_pcre_feats[r] = dn.donor_pcre_feats[r]
        out = _lib.cf_input_grads()
        attr = {}
        for r, b in enumerate(self.binsizes):
            for k, field in (("promoter_feats", out.promoter_feats), ("pcre_feats", out.pcre_feats)):
                if k in inputs:
                    t = attr.setdefault(k, {})[b] = torch.empty(canon[k][b], device=dev)      # (written in full by the library)
                    field[r] = t.data_ptr()
        if "interaction_freq" in inputs:
            t = attr["interaction_freq"] = torch.empty(canon["interaction_freq"], device=dev)
            out.interaction_freq = t.data_ptr()
        lx = torch.empty(B, self.n_out, device=dev)
        lb = torch.empty(B, self.n_out, device=dev)
        delta = torch.empty(B, device=dev)
        st = book()
        info = {"logits": lx, "baseline_logits": lb, "delta": delta}
        if signal:
            co = _lib.cf_input_grads()
            second = "cmean" if donor is not None else "coeff"
            coeff = info[second] = {}
            for r, b in enumerate(self.binsizes):
                for k, field in (("promoter_feats", co.promoter_feats), ("pcre_feats", co.pcre_feats)):
                    if k in inputs:
                        t = coeff.setdefault(k, {})[b] = torch.empty(canon[k][b], device=dev)      # (written in full by the library)
                        field[r] = t.data_ptr()
            if donor is not None:
                _lib.check(_lib.lib().cf_integrated_gradients_raw_donor(self._handle, C.byref(bs), C.byref(opts), C.byref(out), C.byref(co),
                                                                        lx.data_ptr(), lb.data_ptr(), delta.data_ptr(), st),
                           "cf_integrated_gradients_raw_donor")
            else:
                _lib.check(_lib.lib().cf_integrated_gradients_raw(self._handle, C.byref(bs), C.byref(opts), C.byref(out), C.byref(co), lx.data_ptr(),
                                                                  lb.data_ptr(), delta.data_ptr(), st), "cf_integrated_gradients_raw")
        else:
            _lib.check(_lib.lib().cf_integrated_gradients(self._handle, C.byref(bs), C.byref(opts), C.byref(out), lx.data_ptr(), lb.data_ptr(),
                                                          delta.data_ptr(), st), "cf_integrated_gradients")
        if shapes is not None:
            attr = {k: ({b: t.view(shapes[k][b]) for b, t in v.items()} if isinstance(v, dict) else v.view(shapes[k])) for k, v in attr.items()}
            if signal:
                info[second] = {k: {b: t.view(shapes[k][b]) for b, t in v.items()} for k, v in info[second].items()}
        return attr, info

    def _scan_mark_bits(self, who, mark_sets):
        """mark_sets (None: attribution.scan_mark_sets' default) validated -> uint32 [n_sets], bit f of word k set where set k holds mark f."""
        from .attribution import scan_mark_sets
        F = self.n_feats
        mark_sets = scan_mark_sets(mark_sets, F)
        bad = [ms for ms in mark_sets if any(not 0 <= f < min(F, 32) for f in ms)]
        if bad or not mark_sets:
            raise ValueError("%s: mark_sets %s: a non-empty list of sets of mark indices in [0, n_feats = %d)" % (who, bad or "()", F))
        return np.array([sum(1 << f for f in set(ms)) for ms in mark_sets], dtype=np.uint32)

    def _scan_flip(self, who, flip, B):
        """flip ([B] bools, or None) -> a uint8 tensor of B entries on the model's device, or None."""
        if flip is None:
            return None
        flip = torch.as_tensor(flip).to(self._device).ne(0).to(torch.uint8).contiguous()
        if flip.numel() != B:
            raise ValueError("%s: flip has %d entries for a batch of %d genes" % (who, flip.numel(), B))
        return flip

    @torch.no_grad()
    def perturbation_scan(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                          interaction_freq=None, region=0, scale=0.0, width=1, mark_sets=None, flip=None, return_feats=False):
        """In-silico perturbation scan (cf_perturbation_scan): the prediction with the histone marks of a mark set scaled by `scale`
        (0 erases, 2 doubles) in RAW-SIGNAL space over a window of one region -- the promoter (region 0) or pCRE slot j (region
        1 + j) -- for every window and every mark set, from one call -> logits [B, V, n_out] on the model's device, no autograd graph.
        With W = min(n_bins), the bins of the coarsest resolution, V = 1 + n_sets * W:

          [:, 0]                the prediction (model(...) under no_grad, bit-equal)
          [:, 1 + k * W + g]    mark set k over window g: the coarse genomic bins [g, g + width) of the region and the finer bins inside
                                them; a covered feature u = log(1 + mean) becomes log1p(scale * expm1(u)), exactly what binning the
                                scaled signal gives.  Windows past the region's real bins (a short pCRE, a dummy slot, a narrowed
                                promoter) and empty mark sets give [:, 0], bit for bit.

        mark_sets: iterables of mark indices; default each mark alone, then all marks together (n_feats + 1 sets).  flip: [B] bools,
        True where the region is stored mirrored (the dataset mirrors '-' strand promoters, never pCREs): window g then counts from
        the genomic start.  return_feats: also {binsize: [B, V, n_bins, n_feats]}, the features of the scanned region that row (b, v)
        read.  Features must stay below ~80 (expm1 in fp32).  The first argument may also be a packed batch (an engine.Slot or a
        pack_batch result), with nothing after it.  The pass overwrites the activations a grad-enabled model(...) keeps for its
        backward: such a pending backward() raises."""
        bs, _keep, book = self._attrib_call("perturbation_scan", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        F, dev, B = self.n_feats, self._device, bs.B
        bits = self._scan_mark_bits("perturbation_scan", mark_sets)
        W = min(self.n_bins)
        V = 1 + len(bits) * W
        opts = _lib.cf_scan_opts()
        opts.region, opts.width, opts.n_sets, opts.scale = int(region), int(width), len(bits), float(scale)
        opts.mark_sets = bits.ctypes.data
        flip = self._scan_flip("perturbation_scan", flip, B)      # (kept alive until the call below has been issued)
        if flip is not None:
            opts.flip = flip.data_ptr()
        feats = None
        if return_feats:
            feats = {}
            for r, b in enumerate(self.binsizes):
                t = feats[b] = torch.empty(B, V, self.n_bins[r], F, device=dev)      # (written in full by the library)
                opts.feats_out[r] = t.data_ptr()
        logits = torch.empty(B, V, self.n_out, device=dev)      # (written in full by the library)
        st = book()
        _lib.check(_lib.lib().cf_perturbation_scan(self._handle, C.byref(bs), C.byref(opts), logits.data_ptr(), st), "cf_perturbation_scan")
        return (logits, feats) if return_feats else logits

    @torch.no_grad()
    def perturbation_scan_regions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                  interaction_freq=None, regions="all", scale=0.0, width=1, mark_sets=None, flip=None):
        """perturbation_scan of several regions from one call (cf_perturbation_scan_regions) -> (logits [n_reg, B, V, n_out] on the
        model's device, the list of scanned regions in block order).  regions: "all" (0 .. i_max), "pcres" (1 .. i_max) or an iterable
        of region indices (0 the promoter, 1 + j pCRE slot j; sorted, duplicates dropped).  Block q carries the bits of
        perturbation_scan(region=regions[q]) with the same scale, width and mark_sets -- `flip` applies to the promoter block alone
        (pCREs are never stored mirrored).  The promoter block costs what perturbation_scan costs; the variants of a pCRE slot run
        slot-packed: i_max variants share one pass of the Embedding + Pairwise stage, and only the Regulation stack and the head run
        per variant.  mark_sets, the packed forms of the first argument and the effect on a pending backward() are those of
        perturbation_scan; there is no return_feats."""
        from .attribution import scan_regions_expand
        bs, _keep, book = self._attrib_call("perturbation_scan_regions", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        dev, B = self._device, bs.B
        regions = scan_regions_expand(regions, self.i_max, "perturbation_scan_regions")
        bits = self._scan_mark_bits("perturbation_scan_regions", mark_sets)
        V = 1 + len(bits) * min(self.n_bins)
        opts = _lib.cf_scan_regions_opts()
        opts.regions = sum(1 << r for r in regions)
        opts.width, opts.n_sets, opts.scale = int(width), len(bits), float(scale)
        opts.mark_sets = bits.ctypes.data
        flip = self._scan_flip("perturbation_scan_regions", flip, B)      # (kept alive until the call below has been issued)
        if flip is not None:
            opts.flip = flip.data_ptr()
        logits = torch.empty(len(regions), B, V, self.n_out, device=dev)      # (written in full by the library)
        st = book()
        _lib.check(_lib.lib().cf_perturbation_scan_regions(self._handle, C.byref(bs), C.byref(opts), logits.data_ptr(), st),
                   "cf_perturbation_scan_regions")
        return logits, regions

    @torch.no_grad()
    def perturbation_scan_fine(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                               interaction_freq=None, region=0, scale=0.0, width=1, stride=None, start=0, n_windows=None, mark_sets=None,
                               lengths=None, flip=None, return_feats=False):
        """perturbation_scan with windows in bins of the FINEST resolution (cf_perturbation_scan_fine) -> logits [B, V, n_out] on the
        model's device, no autograd graph; V = 1 + n_sets * n_windows:

          [:, 0]                        the prediction (model(...) under no_grad, bit-equal)
          [:, 1 + k * n_windows + g]    mark set k over the finest genomic bins [start[b] + g * stride, start[b] + g * stride + width) of
                                        the region.  A coarser bin the window covers wholly follows perturbation_scan's rule; one it
                                        covers in part is recomputed from its finest children, weighted by their sample counts -- what
                                        binning the scaled signal gives, up to the rounding of the stored features.  Windows past the
                                        region's real bins and empty mark sets give [:, 0], bit for bit.

        width, stride (default: width) in finest bins; start: an int or B ints, the first finest genomic bin per gene (zoom into a
        different coarse window per gene); n_windows: default the windows that reach the end of the region from the smallest start.
        lengths: B ints, the scanned region's length in samples, so that the short last bin of a region is weighted by what it holds
        (None: every real finest bin is full -- exact for promoters and whenever the length is a multiple of the finest bin size;
        giving it costs one read-back of the pad-mask rows and a stream synchronisation).  mark_sets, flip, return_feats, the packed
        forms of the first argument and the effect on a pending backward() are those of perturbation_scan."""
        who = "perturbation_scan_fine"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        F, dev, B = self.n_feats, self._device, bs.B
        bits = self._scan_mark_bits(who, mark_sets)
        Lf = self.n_bins[min(range(len(self.binsizes)), key=lambda r: self.binsizes[r])]
        width = int(width)
        stride = width if stride is None else int(stride)
        start = np.asarray(start, dtype=np.int64).reshape(-1)
        if start.size == 1:
            start = np.repeat(start, B)
        if start.size != B:
            raise ValueError("%s: start has %d entries for a batch of %d genes" % (who, start.size, B))
        if start.size and (start.min() < -2 ** 31 or start.max() >= 2 ** 31):
            raise ValueError("%s: start does not fit an int" % who)
        start = start.astype(np.int32)
        if n_windows is None:
            first = max(int(start.min()), 0) if B else 0
            n_windows = max(-(-(Lf - first) // max(stride, 1)), 1)
        n_windows = int(n_windows)
        V = 1 + len(bits) * max(n_windows, 0)
        opts = _lib.cf_scan_fine_opts()
        opts.region, opts.n_sets, opts.scale = int(region), len(bits), float(scale)
        opts.width, opts.stride, opts.n_windows = width, stride, n_windows
        opts.mark_sets = bits.ctypes.data
        opts.start = start.ctypes.data
        if lengths is not None:
            lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
            if lengths.size != B:
                raise ValueError("%s: lengths has %d entries for a batch of %d genes" % (who, lengths.size, B))
            lengths = np.clip(lengths, -1, 2 ** 31 - 1).astype(np.int32)      # (out of range either way: refused by the library)
            opts.lengths = lengths.ctypes.data
        flip = self._scan_flip(who, flip, B)      # (kept alive until the call below has been issued)
        if flip is not None:
            opts.flip = flip.data_ptr()
        feats = None
        if return_feats:
            feats = {}
            for r, b in enumerate(self.binsizes):
                t = feats[b] = torch.empty(B, V, self.n_bins[r], F, device=dev)      # (written in full by the library)
                opts.feats_out[r] = t.data_ptr()
        logits = torch.empty(B, V, self.n_out, device=dev)      # (written in full by the library)
        st = book()
        _lib.check(_lib.lib().cf_perturbation_scan_fine(self._handle, C.byref(bs), C.byref(opts), logits.data_ptr(), st), "cf_perturbation_scan_fine")
        return (logits, feats) if return_feats else logits

    def perturbation_scan_fine_dataset(self, dataset, genes=None, region="promoter", zoom=None, scale=0.0, width=1, stride=None, mark_sets=None,
                                       target=None, bsz=None, store=None):
        """perturbation_scan_fine over the genes of a ChromoformerDataset with windows in genomic coordinates
        (chromoformer_amd.attribution.perturbation_scan_fine, a generator of per-gene dicts)."""
        from .attribution import perturbation_scan_fine
        return perturbation_scan_fine(self, dataset, genes=genes, region=region, zoom=zoom, scale=scale, width=width, stride=stride,
                                      mark_sets=mark_sets, target=target, bsz=bsz, store=store)

    def perturbation_scan_dataset(self, dataset, genes=None, regions="promoter", scale=0.0, width=1, mark_sets=None, bsz=None, store=None):
        """perturbation_scan over the genes of a ChromoformerDataset with windows in genomic coordinates
        (chromoformer_amd.attribution.perturbation_scan, a generator of per-gene dicts)."""
        from .attribution import perturbation_scan
        return perturbation_scan(self, dataset, genes=genes, regions=regions, scale=scale, width=width, mark_sets=mark_sets, bsz=bsz, store=store)

    def _mark_opts(self, players, scale):
        """players (a mark_players spec) and scale -> (cf_mark_opts, the arrays it points to, names)."""
        from .attribution import mark_players
        marks, regions, names = mark_players(players, self.n_feats, self.i_max)
        opts = _lib.cf_mark_opts()
        opts.n_players, opts.scale = len(marks), float(scale)
        opts.player_marks, opts.player_regions = marks.ctypes.data, regions.ctypes.data
        return opts, (marks, regions), names

    # The four calls every mark game offers, on a checked options struct of its family (`cfn`: the library's entry point): the runners
    # allocate the outputs, book the call, run it and build `info`.
    def _mark_run_coalitions(self, cfn, bs, opts, words, book):
        logits = torch.empty(bs.B, len(words), self.n_out, device=self._device)      # (written in full by the library)
        st = book()
        _lib.check(getattr(_lib.lib(), cfn)(self._handle, C.byref(bs), C.byref(opts), words.ctypes.data, len(words), logits.data_ptr(), st), cfn)
        return logits

    def _mark_run_shapley(self, cfn, bs, opts, names, absent_key, book, return_coalitions):
        P = opts.n_players
        n = 1 << P
        rows = torch.empty(bs.B, n, self.n_out, device=self._device)      # (both written in full by the library)
        phi = torch.empty(bs.B, P, self.n_out, device=self._device)
        st = book()
        _lib.check(getattr(_lib.lib(), cfn)(self._handle, C.byref(bs), C.byref(opts), phi.data_ptr(), rows.data_ptr(), st), cfn)
        info = {"logits": rows[:, n - 1].clone(), absent_key: rows[:, 0].clone(), "players": names}
        info["delta"] = phi.sum(1) - (info["logits"] - info[absent_key])
        if return_coalitions:
            info["coalitions"] = rows
        return phi, info

    def _interactions_info(self, inter, phi, rows, index, absent_key, names, return_coalitions):
        """`info` of an interactions call from its outputs; rows [B, 2^P, n_out], word m at column m."""
        n = rows.shape[1]
        info = {"phi": phi, "logits": rows[:, n - 1].clone(), absent_key: rows[:, 0].clone(), "index": index}
        if names is not None:
            info["players"] = names
        if index == "sti":      # efficiency: the diagonal plus the upper triangle sums to v(N) - v(0)
            P = inter.shape[1]
            upper = torch.triu(torch.ones(P, P, dtype=torch.bool, device=inter.device))
            info["delta"] = inter[:, upper].sum(1) - (info["logits"] - info[absent_key])
        if return_coalitions:
            info["coalitions"] = rows
        return info

    def _mark_run_interactions(self, cfn, bs, opts, names, absent_key, book, index, return_coalitions):
        from .attribution import interaction_index
        code = interaction_index(index, cfn[3:])
        P = opts.n_players
        n = 1 << P
        rows = torch.empty(bs.B, n, self.n_out, device=self._device)      # (all three written in full by the library)
        inter = torch.empty(bs.B, P, P, self.n_out, device=self._device)
        phi = torch.empty(bs.B, P, self.n_out, device=self._device)
        st = book()
        _lib.check(getattr(_lib.lib(), cfn)(self._handle, C.byref(bs), C.byref(opts), code, inter.data_ptr(), phi.data_ptr(), rows.data_ptr(), st), cfn)
        return inter, self._interactions_info(inter, phi, rows, index, absent_key, names, return_coalitions)

    def _mark_run_epistasis(self, cfn, bs, opts, names, book):
        P = opts.n_players
        rows = torch.empty(bs.B, 1 + P + P * (P - 1) // 2, self.n_out, device=self._device)      # (both written in full by the library)
        eps = torch.empty(bs.B, P, P, self.n_out, device=self._device)
        st = book()
        _lib.check(getattr(_lib.lib(), cfn)(self._handle, C.byref(bs), C.byref(opts), eps.data_ptr(), rows.data_ptr(), st), cfn)
        return eps, {"logits": rows[:, 0].clone(), "single": rows[:, 1:1 + P].clone(), "players": names}

    def _permutations(self, who, P, n_perm, seed, permutations):
        """The orders of a sampled game of P players -> uint8 [n_perm, P]: shapley_permutations, or `permutations` checked."""
        from .attribution import shapley_permutations
        if permutations is None:
            return shapley_permutations(P, n_perm, seed)
        given = np.asarray(permutations.cpu() if hasattr(permutations, "cpu") else permutations)
        if given.ndim != 2 or given.shape[0] < 1 or given.shape[1] != P or given.dtype.kind not in "iu" or given.min() < 0 or given.max() >= P:
            raise ValueError("%s: permutations must be an integer array [n_perm >= 1, P = %d] with entries in [0, P)" % (who, P))
        return np.ascontiguousarray(given, dtype=np.uint8)

    def _mark_run_sampled(self, cfn, bs, opts, names, perms, book, return_rows):
        P, n = opts.n_players, len(perms)
        rows = torch.empty(bs.B, 2 + n * (P - 1), self.n_out, device=self._device)      # (all three written in full by the library)
        phi = torch.empty(bs.B, P, self.n_out, device=self._device)
        se = torch.empty(bs.B, P, self.n_out, device=self._device)
        st = book()
        _lib.check(getattr(_lib.lib(), cfn)(self._handle, C.byref(bs), C.byref(opts), perms.ctypes.data, n, phi.data_ptr(), se.data_ptr(),
                                            rows.data_ptr(), st), cfn)
        info = {"logits": rows[:, 1].clone(), "absent": rows[:, 0].clone(), "stderr": se, "names": names, "permutations": perms}
        info["delta"] = phi.sum(1) - (info["logits"] - info["absent"])
        if return_rows:
            info["rows"] = rows
        return phi, info

    def _mark_run_pairs_sampled(self, cfn, bs, opts, names, perms, focal, index, book, return_rows):
        """The sampled interactions call of a wide game (`cfn`) -> (inter, info): see mark_shapley_interactions_sampled."""
        from .attribution import focal_players, focal_row_count, focal_words, interaction_index
        code = interaction_index(index, cfn[3:])
        P, n = opts.n_players, len(perms)
        if P < 2:
            raise ValueError("%s: %d player; a pair needs at least 2" % (cfn[3:], P))
        if focal is None:
            raise ValueError("%s: focal is required: the players whose interactions are asked for (indices or names)" % cfn[3:])
        focal = focal_players(focal, names, P)
        words, col = focal_words(perms, focal)
        F, R, dev = len(focal), len(words), self._device
        rows = torch.empty(bs.B, R, self.n_out, device=dev)      # (all five written in full by the library)
        inter, se = torch.empty(bs.B, F, P, self.n_out, device=dev), torch.empty(bs.B, F, P, self.n_out, device=dev)
        phi, phi_se = torch.empty(bs.B, P, self.n_out, device=dev), torch.empty(bs.B, P, self.n_out, device=dev)
        st = book()
        _lib.check(getattr(_lib.lib(), cfn)(self._handle, C.byref(bs), C.byref(opts), perms.ctypes.data, n, focal.ctypes.data, F, code,
                                            inter.data_ptr(), se.data_ptr(), phi.data_ptr(), phi_se.data_ptr(), rows.data_ptr(), st), cfn)
        at = torch.as_tensor([focal_row_count(perms, focal[:f]) for f in range(F)], device=dev)      # {i} alone; everybody but i follows it
        info = {"stderr": se, "phi": phi, "phi_stderr": phi_se, "logits": rows[:, 1].clone(), "absent": rows[:, 0].clone(),
                "alone": rows[:, at].clone(), "without": rows[:, at + 1].clone(), "index": index, "names": names,
                "focal": focal, "permutations": perms, "col": col, "delta": None}
        if index == "sii":      # every order telescopes: sum_{j != i} d(j) = (v(N) - v(N - i)) - (v({i}) - v(0))
            off = torch.ones(F, P, dtype=torch.bool, device=dev)
            off[torch.arange(F, device=dev), torch.as_tensor(focal.astype(np.int64), device=dev)] = False
            total = (inter * off[None, :, :, None]).sum(2)
            info["delta"] = total - ((info["logits"][:, None] - info["without"]) - (info["alone"] - info["absent"][:, None]))
        if return_rows:
            info["rows"] = rows
        return inter, info

    @torch.no_grad()
    def perm_interactions_from_rows(self, rows, permutations, focal, index="sii"):
        """The reducers of the sampled interactions calls on a table (cf_perm_interactions_from_rows) -> (inter, stderr, phi,
        phi_stderr).  rows: a float32 tensor [B, R, n] on the model's device in the layout of attribution.focal_words(permutations,
        focal) (any n >= 1); permutations: integer [n_perm, P], 2 <= P <= 128; focal: distinct player indices.  inter, stderr
        [B, n_focal, P, n]; phi, phi_stderr [B, P, n].  No forward runs and no activation is written."""
        from .attribution import focal_players, focal_row_count, interaction_index
        who = "perm_interactions_from_rows"
        code = interaction_index(index, who)
        if self._handle is None:
            raise RuntimeError("call .cuda() first: the Chromoformer HIP path needs device buffers")
        perms = np.ascontiguousarray(np.asarray(permutations.cpu() if hasattr(permutations, "cpu") else permutations))
        if perms.ndim != 2 or perms.dtype.kind not in "iu" or not 2 <= perms.shape[1] <= 128 or perms.min() < 0 or perms.max() >= perms.shape[1]:
            raise ValueError("%s: permutations must be an integer array [n_perm >= 1, 2 <= P <= 128] with entries in [0, P)" % who)
        perms = np.ascontiguousarray(perms, dtype=np.uint8)
        n, P = perms.shape
        focal = focal_players(focal, None, P)
        R = focal_row_count(perms, focal)
        if not torch.is_tensor(rows) or rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[1] != R or rows.device != self._device:
            raise ValueError("%s: rows must be a float32 tensor [B, R = %d, n] on %s" % (who, R, self._device))
        rows = rows.contiguous()
        B, n_out, F, dev = rows.shape[0], rows.shape[2], len(focal), self._device
        inter, se = torch.empty(B, F, P, n_out, device=dev), torch.empty(B, F, P, n_out, device=dev)
        phi, phi_se = torch.empty(B, P, n_out, device=dev), torch.empty(B, P, n_out, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib().cf_perm_interactions_from_rows(self._handle, rows.data_ptr(), B, P, n_out, perms.ctypes.data, n, focal.ctypes.data, F,
                                                             code, inter.data_ptr(), se.data_ptr(), phi.data_ptr(), phi_se.data_ptr(), st),
                   "cf_perm_interactions_from_rows")
        return inter, se, phi, phi_se

    @torch.no_grad()
    def mark_coalitions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                        interaction_freq=None, keep=None, players="marks", scale=0.0):
        """The prediction under histone-mark coalitions (cf_mark_coalitions) -> logits [B, n_coal, n_out] on the model's device, no
        autograd graph.  The players are marks, each optionally restricted to regions (attribution.mark_players: "marks",
        "compartments", "regions" or a list of (marks, regions) pairs).  `keep`: a sequence / array of ints, bit p set = player p
        present, or a bool array [n_coal, P].  Column c is the inference forward with the raw signal of every ABSENT player's marks
        scaled by `scale` (0 erases, the default) over the player's regions: a feature u = log(1 + mean) becomes
        log1p(scale * expm1(u)), exactly what binning the scaled signal gives; an element covered by several absent players is scaled
        once.  The full word 2^P - 1 is the prediction (model(...) under no_grad, bit-equal).  Features must stay below ~80 (expm1 in
        fp32).  The first argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.  The
        pass overwrites the activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        from .attribution import mark_coalition_words
        if keep is None:
            raise ValueError("mark_coalitions: keep is required: the coalition words (bit p set: player p present)")
        opts, _alive, _names = self._mark_opts(players, scale)
        words = mark_coalition_words(keep, opts.n_players, "mark_coalitions")
        bs, _keep, book = self._attrib_call("mark_coalitions", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        return self._mark_run_coalitions("cf_mark_coalitions", bs, opts, words, book)

    @torch.no_grad()
    def mark_shapley(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                     interaction_freq=None, players="marks", scale=0.0, return_coalitions=False):
        """Exact Shapley values of the histone marks (cf_mark_shapley) -> (phi, info), tensors on the model's device, no autograd graph:

          phi                 [B, P, n_out]: player p's average marginal contribution to each logit over all orders of adding the
                              players to the gene with every player absent; exactly 0 for a player whose elements are all zeros
          info["logits"]      [B, n_out]: the prediction (every player present; model(...) under no_grad, bit-equal)
          info["erased"]      [B, n_out]: every player absent
          info["delta"]       [B, n_out]: phi.sum(1) - (logits - erased), the efficiency gap (rounding only)
          info["players"]     the players' names
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        players and scale as in mark_coalitions; all 2^P coalitions (128 for the seven marks) run from one call, in logit space, where
        efficiency holds.  The packed forms of the first argument and the effect on a pending backward() are those of mark_coalitions."""
        opts, _alive, names = self._mark_opts(players, scale)
        bs, _keep, book = self._attrib_call("mark_shapley", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        return self._mark_run_shapley("cf_mark_shapley", bs, opts, names, "erased", book, return_coalitions)

    @torch.no_grad()
    def mark_epistasis(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                       interaction_freq=None, players="marks", scale=0.0):
        """Pair epistasis of the histone-mark players (cf_mark_epistasis) -> (eps, info), tensors on the model's device, no autograd
        graph.  With v(...) the logits with the named players absent:

          eps[:, i, j]    [B, P, P, n_out]: ((v() - v(i)) - v(j)) + v(i, j) for i != j, exactly symmetric: 0 when the two marks add
                          up, non-zero when they are redundant or cooperate; eps[:, i, i] = v() - v(i), the leave-one-out effect
          info["logits"]  [B, n_out]: v(), the prediction;  info["single"]  [B, P, n_out]: v(i);  info["players"]  the names

        The 1 + P + P (P - 1) / 2 rows (attribution.coalition_table("pairs", P)) run from one call.  players, scale, the packed forms
        of the first argument and the effect on a pending backward() are those of mark_coalitions."""
        opts, _alive, names = self._mark_opts(players, scale)
        bs, _keep, book = self._attrib_call("mark_epistasis", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        return self._mark_run_epistasis("cf_mark_epistasis", bs, opts, names, book)

    @torch.no_grad()
    def mark_shapley_interactions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                  interaction_freq=None, players="marks", scale=0.0, index="sii", return_coalitions=False):
        """Pairwise Shapley interaction indices of the histone-mark players (cf_mark_shapley_interactions) -> (inter, info), tensors on
        the model's device, no autograd graph.  At least 2 players; the 2^P coalitions run once, as in mark_shapley:

          inter               [B, P, P, n_out], exactly symmetric.  Off the diagonal, with S over the coalitions that hold neither player,
                              I_ij = sum_S w(|S|) ((v(S + i + j) - v(S + j)) - (v(S + i) - v(S))): how much i's marginal contribution
                              changes with j present, averaged over every context -- negative for redundant players, positive for
                              cooperating ones, also where a third player hides the effect from the full-coalition *_epistasis.  index "sii"
                              (Shapley interaction index): w(s) = s! (P - s - 2)! / (P - 1)!, the diagonal is phi.  index "sti"
                              (Shapley-Taylor, order 2): w(s) = (2 / P) / C(P - 1, s), the diagonal is v({i}) - v(nobody), and the
                              diagonal plus the upper triangle sums to logits - erased.  A null player's row and column are exactly 0
          info["phi"]         [B, P, n_out]: the Shapley values of mark_shapley on the same rows, bit for bit
          info["logits"]      [B, n_out]: the prediction;  info["erased"]  [B, n_out]: every player absent
          info["index"]       the index name;  info["delta"]  [B, n_out], "sti" only: the efficiency gap (rounding only)
          info["players"]     the players' names
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        SHAP's interaction values follow from the sii result: Phi_ij = I_ij / 2 off the diagonal and Phi_ii = phi_i - sum_{j != i} I_ij / 2.
        players and scale as in mark_coalitions.  The packed forms of the first argument and the effect on a pending backward() are
        those of mark_coalitions."""
        opts, _alive, names = self._mark_opts(players, scale)
        bs, _keep, book = self._attrib_call("mark_shapley_interactions", (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        return self._mark_run_interactions("cf_mark_shapley_interactions", bs, opts, names, "erased", book, index, return_coalitions)

    def mark_shapley_dataset(self, dataset, genes=None, players="marks", scale=0.0, epistasis=False, bsz=None, store=None, interactions=None,
                             dividends=False):
        """mark_shapley (and optionally mark_epistasis, or mark_shapley_interactions in its place; with dividends=True the Harsanyi
        dividends of the same table too) over the genes of a ChromoformerDataset (chromoformer_amd.attribution.mark_shapley, a generator
        of per-gene dicts)."""
        from .attribution import mark_shapley
        return mark_shapley(self, dataset, genes=genes, players=players, scale=scale, epistasis=epistasis, bsz=bsz, store=store,
                            interactions=interactions, dividends=dividends)

    def _mark_donor_opts(self, who, donor, players, B):
        """players (a mark_players spec) and the donor of a batch of B genes -> (cf_mark_donor_opts, what it points to, names).  donor:
        a (promoter_feats, pcre_feats) pair of dicts by bin size (or lists in binsizes order) of contiguous float32 tensors on the
        model's device, [B, 1, L, F] and [B, i_max, L, F]; or a packed batch (an engine.Slot, a pack_batch result or a batch struct),
        whose features are used and the rest ignored.  Anything else raises ValueError naming `who`."""
        from .attribution import mark_players
        marks, regions, names = mark_players(players, self.n_feats, self.i_max)
        opts = _lib.cf_mark_donor_opts()
        opts.n_players = len(marks)
        opts.player_marks, opts.player_regions = marks.ctypes.data, regions.ctypes.data
        return opts, (marks, regions) + self._donor_feats(who, donor, B, opts), names

    def _donor_feats(self, who, donor, B, opts):
        """The donor of a batch of B genes (the forms of _mark_donor_opts) checked, its feature pointers written into
        opts.donor_promoter_feats / donor_pcre_feats -> what they point to."""
        if donor is None:
            raise ValueError("%s: donor is required: the same genes' features in the other cell type, a (promoter_feats, pcre_feats) "
                             "pair or a packed batch" % who)
        S, F = self.i_max, self.n_feats
        packed = donor if isinstance(donor, _lib.cf_batch) else getattr(donor, "struct", None)
        if packed is None and isinstance(donor, (tuple, list)) and len(donor) == 2 and isinstance(donor[0], _lib.cf_batch):
            packed = donor[0]
        if packed is not None:
            if packed.B != B:
                raise ValueError("%s: the donor holds %d genes, the batch %d" % (who, packed.B, B))
            for r in range(len(self.binsizes)):
                opts.donor_promoter_feats[r], opts.donor_pcre_feats[r] = packed.promoter_feats[r], packed.pcre_feats[r]
            return (donor,)
        try:
            pfs, cfs = donor
            pfs = [pfs[b] for b in self.binsizes] if isinstance(pfs, dict) else list(pfs)
            cfs = [cfs[b] for b in self.binsizes] if isinstance(cfs, dict) else list(cfs)
        except (TypeError, ValueError, KeyError):
            raise ValueError("%s: donor must be a (promoter_feats, pcre_feats) pair of dicts by bin size %s (or lists in that order) or a "
                             "packed batch" % (who, list(self.binsizes))) from None
        if len(pfs) != len(self.binsizes) or len(cfs) != len(self.binsizes):
            raise ValueError("%s: donor has %d / %d feature tensors, the model %d resolutions" % (who, len(pfs), len(cfs), len(self.binsizes)))
        for r, b in enumerate(self.binsizes):
            L = self.n_bins[r]
            for name, t, lead in (("promoter_feats", pfs[r], 1), ("pcre_feats", cfs[r], S)):
                what = "%s: donor %s[%d]" % (who, name, b)
                if not torch.is_tensor(t):
                    raise ValueError("%s is not a tensor" % what)
                if t.dtype != torch.float32:
                    raise ValueError("%s is %s; the donor's bits are selected as they are: float32 is required" % (what, t.dtype))
                if t.device != self._device:
                    raise ValueError("%s is on %s, the model on %s" % (what, t.device, self._device))
                if t.numel() != B * lead * L * F or t.dim() < 3 or t.shape[0] != B or tuple(t.shape[-2:]) != (L, F):
                    raise ValueError("%s has shape %s; expected %s" % (what, tuple(t.shape), (B, lead, L, F)))
                if not t.is_contiguous():
                    raise ValueError("%s is not contiguous" % what)
            opts.donor_promoter_feats[r], opts.donor_pcre_feats[r] = pfs[r].data_ptr(), cfs[r].data_ptr()
        return (pfs, cfs)

    @torch.no_grad()
    def mark_donor_coalitions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                              interaction_freq=None, donor=None, keep=None, players="marks"):
        """The prediction under histone-mark coalitions against a donor cell type (cf_mark_donor_coalitions) -> logits
        [B, n_coal, n_out] on the model's device, no autograd graph.  Players and `keep` as in mark_coalitions.  `donor`: the same B
        genes' features in the other cell type -- a (promoter_feats, pcre_feats) pair of dicts by bin size (or lists in binsizes
        order) of contiguous float32 tensors on the model's device, or a packed batch (an engine.Slot or a pack_batch result), whose
        features are used and the rest ignored.  Column c is the inference forward with every ABSENT player's marks taken from the
        donor over the player's regions, bit for bit, at every resolution and in every row; masks and interaction_freq stay the
        gene's own.  Where the two cell types share a region's coordinates this is exactly what binning the raw region with those
        marks' rows replaced gives.  The full word 2^P - 1 is the prediction (model(...) under no_grad, bit-equal).  The first
        argument may also be a packed batch, with nothing after it.  The pass overwrites the activations a grad-enabled model(...)
        keeps for its backward: such a pending backward() raises."""
        from .attribution import mark_coalition_words
        who = "mark_donor_coalitions"
        if keep is None:
            raise ValueError("mark_donor_coalitions: keep is required: the coalition words (bit p set: player p present)")
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, _names = self._mark_donor_opts(who, donor, players, bs.B)
        return self._mark_run_coalitions("cf_mark_donor_coalitions", bs, opts, mark_coalition_words(keep, opts.n_players, who), book)

    @torch.no_grad()
    def mark_donor_shapley(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                           interaction_freq=None, donor=None, players="marks", return_coalitions=False):
        """Exact Shapley values of the histone marks against a donor cell type (cf_mark_donor_shapley) -> (phi, info), tensors on the
        model's device, no autograd graph: which mark changes account for the difference between the two predictions?

          phi                 [B, P, n_out]: player p's average marginal contribution to each logit over all orders of switching the
                              players from the donor's signal to the gene's; exactly 0 for a player whose elements are the same in both
          info["logits"]      [B, n_out]: the prediction (every player present; model(...) under no_grad, bit-equal)
          info["donor"]       [B, n_out]: every player absent: the donor's marks under the gene's masks and frequencies
          info["delta"]       [B, n_out]: phi.sum(1) - (logits - donor), the efficiency gap (rounding only)
          info["players"]     the players' names
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        donor and players as in mark_donor_coalitions; all 2^P coalitions run from one call.  The packed forms of the first argument
        and the effect on a pending backward() are those of mark_coalitions."""
        who = "mark_donor_shapley"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, names = self._mark_donor_opts(who, donor, players, bs.B)
        return self._mark_run_shapley("cf_mark_donor_shapley", bs, opts, names, "donor", book, return_coalitions)

    @torch.no_grad()
    def mark_donor_epistasis(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                             interaction_freq=None, donor=None, players="marks"):
        """Pair epistasis of the histone-mark players against a donor cell type (cf_mark_donor_epistasis) -> (eps, info) as
        mark_epistasis returns them, with v(...) the logits with the named players' marks taken from the donor.  donor and players as
        in mark_donor_coalitions."""
        who = "mark_donor_epistasis"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, names = self._mark_donor_opts(who, donor, players, bs.B)
        return self._mark_run_epistasis("cf_mark_donor_epistasis", bs, opts, names, book)

    @torch.no_grad()
    def mark_donor_shapley_interactions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                        interaction_freq=None, donor=None, players="marks", index="sii", return_coalitions=False):
        """Pairwise Shapley interaction indices of the histone-mark players against a donor cell type
        (cf_mark_donor_shapley_interactions) -> (inter, info), tensors on the model's device, no autograd graph.  At least 2 players;
        the 2^P coalitions run once, as in mark_donor_shapley:

          inter               [B, P, P, n_out], exactly symmetric.  Off the diagonal, with S over the coalitions that hold neither player,
                              I_ij = sum_S w(|S|) ((v(S + i + j) - v(S + j)) - (v(S + i) - v(S))): how much i's marginal contribution
                              changes with j present, averaged over every context -- negative for redundant players, positive for
                              cooperating ones, also where a third player hides the effect from the full-coalition *_epistasis.  index "sii"
                              (Shapley interaction index): w(s) = s! (P - s - 2)! / (P - 1)!, the diagonal is phi.  index "sti"
                              (Shapley-Taylor, order 2): w(s) = (2 / P) / C(P - 1, s), the diagonal is v({i}) - v(nobody), and the
                              diagonal plus the upper triangle sums to logits - donor.  A null player's row and column are exactly 0
          info["phi"]         [B, P, n_out]: the Shapley values of mark_donor_shapley on the same rows, bit for bit
          info["logits"]      [B, n_out]: the prediction;  info["donor"]  [B, n_out]: every player absent
          info["index"]       the index name;  info["delta"]  [B, n_out], "sti" only: the efficiency gap (rounding only)
          info["players"]     the players' names
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        SHAP's interaction values follow from the sii result: Phi_ij = I_ij / 2 off the diagonal and Phi_ii = phi_i - sum_{j != i} I_ij / 2.
        donor and players as in mark_donor_coalitions; a player whose elements are the same in both cell types is a null player."""
        who = "mark_donor_shapley_interactions"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, names = self._mark_donor_opts(who, donor, players, bs.B)
        return self._mark_run_interactions("cf_mark_donor_shapley_interactions", bs, opts, names, "donor", book, index, return_coalitions)

    def mark_donor_shapley_dataset(self, dataset, donor_dataset, genes=None, players="marks", epistasis=False, bsz=None, store=None, donor_store=None,
                                   interactions=None, dividends=False):
        """mark_donor_shapley (and optionally mark_donor_epistasis, the interaction index, the dividends) over the genes of two
        ChromoformerDatasets, the gene's cell type and the donor's (chromoformer_amd.attribution.mark_donor_shapley, a generator of
        per-gene dicts)."""
        from .attribution import mark_donor_shapley
        return mark_donor_shapley(self, dataset, donor_dataset, genes=genes, players=players, epistasis=epistasis, bsz=bsz, store=store,
                                  donor_store=donor_store, interactions=interactions, dividends=dividends)

    def _mark_wide_opts(self, who, players, scale, donor, B):
        """players (a mark_players_wide spec), scale and donor (None: the scale rule; else the forms of _mark_donor_opts) for a batch of
        B genes -> (cf_mark_wide_opts, what it points to, names)."""
        from .attribution import mark_players_wide
        marks, regions, names = mark_players_wide(players, self.n_feats, self.i_max)
        opts = _lib.cf_mark_wide_opts()
        opts.n_players, opts.scale = len(marks), float(scale)
        opts.player_marks, opts.player_regions = marks.ctypes.data, regions.ctypes.data
        alive = (marks, regions) + (self._donor_feats(who, donor, B, opts) if donor is not None else ())
        return opts, alive, names

    @torch.no_grad()
    def mark_coalitions_wide(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                             interaction_freq=None, keep=None, players="cells", scale=0.0, donor=None):
        """The prediction under histone-mark coalitions of up to 128 players (cf_mark_coalitions_wide) -> logits [B, n_coal, n_out] on
        the model's device, no autograd graph.  players: attribution.mark_players_wide -- what mark_coalitions takes, or "cells", one
        player per (mark, region) pair: n_feats (i_max + 1) of them.  `keep`: a bool array [n_coal, P], or a sequence of Python ints
        (bit p set = player p present; attribution.mark_wide_words).  donor None: an ABSENT player's raw signal is scaled by `scale`
        (0 erases) as in mark_coalitions; a donor (the forms of mark_donor_coalitions): its elements take the donor's bits and `scale`
        is not read.  With at most 16 players the rows carry the bits of mark_coalitions / mark_donor_coalitions.  The packed forms
        of the first argument and the effect on a pending backward() are those of mark_coalitions."""
        from .attribution import mark_wide_words
        who = "mark_coalitions_wide"
        if keep is None:
            raise ValueError("mark_coalitions_wide: keep is required: the coalitions (bit p set: player p present)")
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, _names = self._mark_wide_opts(who, players, scale, donor, bs.B)
        return self._mark_run_coalitions("cf_mark_coalitions_wide", bs, opts, mark_wide_words(keep, opts.n_players, who), book)

    @torch.no_grad()
    def mark_shapley_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                             interaction_freq=None, players="cells", n_perm=64, seed=0, permutations=None, scale=0.0, donor=None,
                             return_rows=False):
        """Permutation-sampled Shapley values of up to 128 histone-mark players (cf_mark_shapley_sampled) -> (phi, info), tensors on the
        model's device, no autograd graph: which mark matters at which region?

          phi                   [B, P, n_out]: the mean, over the sampled orders of adding the players, of player p's marginal
                                contribution to each logit; exactly 0 for a player whose elements are the same present and absent.
                                With players="cells", phi.view(B, i_max + 1, n_feats, n_out)[:, rho, f] is mark f in region rho
          info["stderr"]        [B, P, n_out]: the standard error of that mean over the orders (0 with one order).  phi is an
                                ESTIMATE: this is the only statement about its sampling error, nothing bounds it
          info["logits"]        [B, n_out]: the prediction (every player present; model(...) under no_grad, bit-equal)
          info["absent"]        [B, n_out]: every player absent (erased, scaled, or the donor's marks)
          info["delta"]         [B, n_out]: phi.sum(1) - (logits - absent), the efficiency gap (rounding only: every order telescopes)
          info["names"]         the players' names
          info["permutations"]  uint8 [n_perm, P]: the orders used
          info["rows"]          [B, 2 + n_perm (P - 1), n_out], with return_rows: nobody, everybody, then per order q its first
                                k = 1 .. P - 1 players at column 2 + q (P - 1) + (k - 1)

        The orders are attribution.shapley_permutations(P, n_perm, seed), or `permutations` (an integer array [n_perm, P], each row a
        permutation; stderr then still assumes independent orders).  players, scale and donor as in mark_coalitions_wide.  The packed
        forms of the first argument and the effect on a pending backward() are those of mark_coalitions."""
        who = "mark_shapley_sampled"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, names = self._mark_wide_opts(who, players, scale, donor, bs.B)
        perms = self._permutations(who, opts.n_players, n_perm, seed, permutations)
        return self._mark_run_sampled("cf_mark_shapley_sampled", bs, opts, names, perms, book, return_rows)

    def mark_shapley_sampled_dataset(self, dataset, donor_dataset=None, genes=None, players="cells", n_perm=64, seed=0, scale=0.0, bsz=None,
                                     store=None, donor_store=None):
        """mark_shapley_sampled over the genes of a ChromoformerDataset, against a donor cell type's dataset if one is given
        (chromoformer_amd.attribution.mark_shapley_sampled, a generator of per-gene dicts)."""
        from .attribution import mark_shapley_sampled
        return mark_shapley_sampled(self, dataset, donor_dataset, genes=genes, players=players, n_perm=n_perm, seed=seed, scale=scale, bsz=bsz,
                                    store=store, donor_store=donor_store)

    @torch.no_grad()
    def mark_shapley_interactions_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None,
                                          interaction_masks=None, interaction_freq=None, players="cells", focal=None, index="sii", n_perm=64,
                                          seed=0, permutations=None, scale=0.0, donor=None, return_rows=False):
        """Permutation-sampled pairwise Shapley interaction indices of a few FOCAL players of up to 128 histone-mark players
        (cf_mark_shapley_interactions_sampled) -> (inter, info), tensors on the model's device, no autograd graph: for the cells that
        carry the prediction (mark_shapley_sampled finds them), which other cells are redundant with them, which cooperate?

          inter                 [B, n_focal, P, n_out]: inter[b, f, j] estimates the interaction index of focal player i = focal[f] with
                                player j -- how much i's marginal contribution changes with j present: per order, with the players
                                that precede j among the others as context, (i's marginal with j) - (i's marginal without j); the mean
                                over the orders.  index "sii": unbiased for the Shapley interaction index; the diagonal j = i is
                                info["phi"][b, i], bit for bit.  index "sti": each sample weighted by 2 (P - 1 - a) / P, a the size of
                                the context: unbiased for Shapley-Taylor of order 2; the diagonal is v({i}) - v(nobody).  Exactly 0
                                where i or j is a null player.  NOT symmetric: inter[b, f, j] from focal i and the entry of focal j at
                                player i are different samples of the same quantity
          info["stderr"]        [B, n_focal, P, n_out]: the standard error of that mean over the orders (0 with one order; 0 on the
                                "sti" diagonal).  inter is an ESTIMATE: this is the only statement about its sampling error
          info["phi"], info["phi_stderr"]   [B, P, n_out]: mark_shapley_sampled's estimate of every player on the same orders, from the
                                same forwards, bit for bit
          info["logits"], info["absent"]    [B, n_out]: everybody present (the prediction), nobody present
          info["alone"], info["without"]    [B, n_focal, n_out]: the focal player alone present; everybody but the focal player
          info["delta"]         [B, n_focal, n_out], "sii": sum_{j != i} inter - ((logits - without) - (alone - absent)), rounding only
                                (every order telescopes); None for "sti"
          info["names"], info["focal"], info["index"], info["permutations"]   the players' names, the focal indices (int32), the index
                                name, the orders (uint8 [n_perm, P])
          info["col"]           uint32 [n_focal, n_perm, P, 2]: the rows the reducer reads (attribution.focal_words)
          info["rows"]          [B, R, n_out], with return_rows: mark_shapley_sampled's table, then the focal players' own rows
                                (attribution.focal_words) -- about as many forwards again as the Shapley estimate per focal player

        focal: player indices or names (attribution.focal_players), distinct.  players, n_perm, seed, permutations, scale and donor as
        in mark_shapley_sampled.  The packed forms of the first argument and the effect on a pending backward() are those of
        mark_coalitions."""
        who = "mark_shapley_interactions_sampled"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, names = self._mark_wide_opts(who, players, scale, donor, bs.B)
        perms = self._permutations(who, opts.n_players, n_perm, seed, permutations)
        return self._mark_run_pairs_sampled("cf_mark_shapley_interactions_sampled", bs, opts, names, perms, focal, index, book, return_rows)

    def mark_shapley_interactions_sampled_dataset(self, dataset, donor_dataset=None, genes=None, players="cells", top=4, focal=None, index="sii",
                                                  n_perm=64, seed=0, scale=0.0, bsz=None, store=None, donor_store=None):
        """mark_shapley_interactions_sampled over the genes of a ChromoformerDataset, the focal players chosen per gene
        (chromoformer_amd.attribution.mark_shapley_interactions_sampled, a generator of per-gene dicts)."""
        from .attribution import mark_shapley_interactions_sampled
        return mark_shapley_interactions_sampled(self, dataset, donor_dataset, genes=genes, players=players, top=top, focal=focal, index=index,
                                                 n_perm=n_perm, seed=seed, scale=scale, bsz=bsz, store=store, donor_store=donor_store)

    def _mark_window_opts(self, who, players, width, scale, donor, flip, B):
        """players (a window_players spec) at `width`, scale, donor (None: the scale rule; else the forms of _mark_donor_opts) and flip
        ([B] bools or None: the promoter is stored mirrored) for a batch of B genes -> (cf_mark_window_opts, what it points to, names)."""
        from .attribution import window_players
        marks, regions, lo, hi, names = window_players(players, self.n_feats, self.i_max, min(self.n_bins), width)
        opts = _lib.cf_mark_window_opts()
        opts.n_players, opts.scale = len(marks), float(scale)
        opts.player_marks, opts.player_regions = marks.ctypes.data, regions.ctypes.data
        opts.player_lo, opts.player_hi = lo.ctypes.data, hi.ctypes.data
        flip = self._scan_flip(who, flip, B)
        if flip is not None:
            opts.flip = flip.data_ptr()
        alive = (marks, regions, lo, hi, flip) + (self._donor_feats(who, donor, B, opts) if donor is not None else ())
        return opts, alive, names

    @torch.no_grad()
    def mark_window_coalitions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                               interaction_freq=None, keep=None, players="promoter", width=1, scale=0.0, donor=None, flip=None):
        """The prediction under coalitions of WINDOW players (cf_mark_window_coalitions) -> logits [B, n_coal, n_out] on the model's
        device, no autograd graph.  A player is a set of marks in a set of regions over a window of bins of the coarsest resolution
        (attribution.window_players: "promoter", "promoter_cells", "regions" at `width` bins per window, or (marks, regions, (lo, hi))
        triples; at most 128).  `keep` as in mark_coalitions_wide.  Column c is the inference forward with the marks of every ABSENT
        player, inside its window of its regions, scaled by `scale` in raw-signal space (0 erases; donor None) or taken from the donor
        (the forms of mark_donor_coalitions), at every resolution; an element covered by several absent players changes once.  flip:
        [B] bools, True where the promoter is stored mirrored ('-' strand): windows count from the genomic start, as in
        perturbation_scan.  One absent single-region player gives the row of perturbation_scan(width=hi - lo) at window lo, bit for bit; a
        window past a region's real bins changes nothing.  The packed forms of the first argument and the effect on a pending
        backward() are those of mark_coalitions."""
        from .attribution import mark_wide_words
        who = "mark_window_coalitions"
        if keep is None:
            raise ValueError("mark_window_coalitions: keep is required: the coalitions (bit p set: player p present)")
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, _names = self._mark_window_opts(who, players, width, scale, donor, flip, bs.B)
        return self._mark_run_coalitions("cf_mark_window_coalitions", bs, opts, mark_wide_words(keep, opts.n_players, who), book)

    @torch.no_grad()
    def mark_window_shapley(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                            interaction_freq=None, players="promoter", width=1, scale=0.0, donor=None, flip=None, return_coalitions=False):
        """Exact Shapley values of at most 16 window players (cf_mark_window_shapley) -> (phi, info), tensors on the model's device, no
        autograd graph: which stretch of the region carries the prediction?  Two redundant stretches share the credit here, where a
        leave-one-out scan scores both near zero.

          phi                 [B, P, n_out]: player p's average marginal contribution over all orders; exactly 0 for a null player
                              (a window past the region's real bins, a dummy slot)
          info["logits"]      [B, n_out]: the prediction (every player present; model(...) under no_grad, bit-equal)
          info["erased"]      [B, n_out]: every player absent (donor None); info["donor"] with a donor
          info["delta"]       [B, n_out]: phi.sum(1) - (logits - erased), the efficiency gap (rounding only)
          info["players"]     the players' names
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        players, width, scale, donor and flip as in mark_window_coalitions."""
        who = "mark_window_shapley"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, names = self._mark_window_opts(who, players, width, scale, donor, flip, bs.B)
        P = opts.n_players
        if P > 16:
            raise ValueError("%s: %d players; the exact game takes 1..16: choose a larger width or mark_window_shapley_sampled" % (who, P))
        return self._mark_run_shapley("cf_mark_window_shapley", bs, opts, names, "erased" if donor is None else "donor", book, return_coalitions)

    @torch.no_grad()
    def mark_window_shapley_interactions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                         interaction_freq=None, players="promoter", width=1, scale=0.0, donor=None, flip=None, index="sii",
                                         return_coalitions=False):
        """Pairwise Shapley interaction indices of 2..16 window players (cf_mark_window_shapley_interactions) -> (inter, info),
        tensors on the model's device, no autograd graph: which stretches are redundant, which cooperate?  The 2^P coalitions run once,
        as in mark_window_shapley:

          inter               [B, P, P, n_out], exactly symmetric.  Off the diagonal, with S over the coalitions that hold neither player,
                              I_ij = sum_S w(|S|) ((v(S + i + j) - v(S + j)) - (v(S + i) - v(S))): how much i's marginal contribution
                              changes with j present, averaged over every context -- negative for redundant players, positive for
                              cooperating ones, also where a third player hides the effect from the full-coalition *_epistasis.  index "sii"
                              (Shapley interaction index): w(s) = s! (P - s - 2)! / (P - 1)!, the diagonal is phi.  index "sti"
                              (Shapley-Taylor, order 2): w(s) = (2 / P) / C(P - 1, s), the diagonal is v({i}) - v(nobody), and the
                              diagonal plus the upper triangle sums to logits - erased.  A null player's row and column are exactly 0
          info["phi"]         [B, P, n_out]: the Shapley values of mark_window_shapley on the same rows, bit for bit
          info["logits"]      [B, n_out]: the prediction;  info["erased"]  [B, n_out]: every player absent
          info["index"]       the index name;  info["delta"]  [B, n_out], "sti" only: the efficiency gap (rounding only)
          info["players"]     the players' names
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        SHAP's interaction values follow from the sii result: Phi_ij = I_ij / 2 off the diagonal and Phi_ii = phi_i - sum_{j != i} I_ij / 2.
        info["donor"] takes the place of info["erased"] with a donor.  players, width, scale, donor and flip as in
        mark_window_coalitions; a window past the region's real bins and a player in a dummy slot are null players."""
        who = "mark_window_shapley_interactions"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, names = self._mark_window_opts(who, players, width, scale, donor, flip, bs.B)
        P = opts.n_players
        if P > 16:
            raise ValueError("%s: %d players; the exact game takes 2..16 and the index has no sampled estimator: choose a larger width" % (who, P))
        return self._mark_run_interactions("cf_mark_window_shapley_interactions", bs, opts, names, "erased" if donor is None else "donor", book,
                                           index, return_coalitions)

    @torch.no_grad()
    def mark_window_shapley_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                    interaction_freq=None, players="promoter", width=1, n_perm=64, seed=0, permutations=None, scale=0.0,
                                    donor=None, flip=None, return_rows=False):
        """Permutation-sampled Shapley values of up to 128 window players (cf_mark_window_shapley_sampled) -> (phi, info) with the keys,
        the row layout and the estimator of mark_shapley_sampled: which mark in which stretch?  players, width, scale, donor and flip
        as in mark_window_coalitions; n_perm, seed and permutations as in mark_shapley_sampled.  A null player (a window past the
        region's real bins, a dummy slot) has phi and stderr exactly 0."""
        who = "mark_window_shapley_sampled"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, names = self._mark_window_opts(who, players, width, scale, donor, flip, bs.B)
        perms = self._permutations(who, opts.n_players, n_perm, seed, permutations)
        return self._mark_run_sampled("cf_mark_window_shapley_sampled", bs, opts, names, perms, book, return_rows)

    @torch.no_grad()
    def mark_window_shapley_interactions_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None,
                                                 interaction_masks=None, interaction_freq=None, players="promoter", width=1, focal=None,
                                                 index="sii", n_perm=64, seed=0, permutations=None, scale=0.0, donor=None, flip=None,
                                                 return_rows=False):
        """Permutation-sampled pairwise Shapley interaction indices of focal players among up to 128 window players
        (cf_mark_window_shapley_interactions_sampled) -> (inter, info) with the keys, the row layout and the estimator of
        mark_shapley_interactions_sampled: which stretches are redundant with the ones that carry the prediction?  players, width,
        scale, donor and flip as in mark_window_coalitions; focal, index, n_perm, seed and permutations as in
        mark_shapley_interactions_sampled.  The estimate is not symmetric; a null player (a window past the region's real bins, a
        dummy slot) has its row and column exactly 0."""
        who = "mark_window_shapley_interactions_sampled"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        opts, _alive, names = self._mark_window_opts(who, players, width, scale, donor, flip, bs.B)
        perms = self._permutations(who, opts.n_players, n_perm, seed, permutations)
        return self._mark_run_pairs_sampled("cf_mark_window_shapley_interactions_sampled", bs, opts, names, perms, focal, index, book, return_rows)

    def mark_window_shapley_dataset(self, dataset, donor_dataset=None, genes=None, players="promoter", width=1, n_perm=64, seed=0, scale=0.0,
                                    bsz=None, store=None, donor_store=None, interactions=None, dividends=False):
        """Shapley values of window players over the genes of a ChromoformerDataset, against a donor cell type's dataset if one is
        given, windows in genomic coordinates (chromoformer_amd.attribution.mark_window_shapley, a generator of per-gene dicts)."""
        from .attribution import mark_window_shapley
        return mark_window_shapley(self, dataset, donor_dataset, genes=genes, players=players, width=width, n_perm=n_perm, seed=seed,
                                   scale=scale, bsz=bsz, store=store, donor_store=donor_store, interactions=interactions, dividends=dividends)

    def _mark_fine_opts(self, who, B, region, players, width, n_windows, start, lengths, scale, donor, flip):
        """The options of the fine window game for a batch of B genes -> (P, cf_mark_fine_opts, what it points to, names)."""
        from .attribution import fine_window_players
        Lf = self.n_bins[min(range(len(self.binsizes)), key=lambda r: self.binsizes[r])]
        start = np.asarray(start, dtype=np.int64).reshape(-1)
        if start.size == 1:
            start = np.repeat(start, B)
        if start.size != B:
            raise ValueError("%s: start has %d entries for a batch of %d genes" % (who, start.size, B))
        if start.size and (start.min() < -2 ** 31 or start.max() >= 2 ** 31):
            raise ValueError("%s: start does not fit an int" % who)
        start = start.astype(np.int32)
        width = int(width)
        if n_windows is None:
            first = max(int(start.min()), 0) if B else 0
            n_windows = max(-(-(Lf - first) // max(width, 1)), 1)
        marks, lo, hi, names = fine_window_players(players, self.n_feats, width, n_windows)
        opts = _lib.cf_mark_fine_opts()
        opts.region, opts.n_players, opts.scale = int(region), len(marks), float(scale)
        opts.player_marks, opts.player_lo, opts.player_hi = marks.ctypes.data, lo.ctypes.data, hi.ctypes.data
        opts.start = start.ctypes.data
        if lengths is not None:
            lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
            if lengths.size != B:
                raise ValueError("%s: lengths has %d entries for a batch of %d genes" % (who, lengths.size, B))
            lengths = np.clip(lengths, -1, 2 ** 31 - 1).astype(np.int32)      # (out of range either way: refused by the library)
            opts.lengths = lengths.ctypes.data
        flip = self._scan_flip(who, flip, B)
        if flip is not None:
            opts.flip = flip.data_ptr()
        alive = (marks, lo, hi, start, lengths, flip) + (self._donor_feats(who, donor, B, opts) if donor is not None else ())
        return len(marks), opts, alive, names

    def _fine_feats(self, opts, B, rows):
        """feats_out of a fine game of `rows` rows per gene, attached to its options -> {binsize: [B, rows, n_bins, n_feats]}."""
        feats = {}
        for r, b in enumerate(self.binsizes):
            t = feats[b] = torch.empty(B, rows, self.n_bins[r], self.n_feats, device=self._device)      # (written in full by the library)
            opts.feats_out[r] = t.data_ptr()
        return feats

    @torch.no_grad()
    def mark_fine_window_coalitions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                    interaction_freq=None, keep=None, region=0, players="windows", width=1, n_windows=None, start=0,
                                    lengths=None, scale=0.0, donor=None, flip=None, return_feats=False):
        """The prediction under coalitions of FINE window players (cf_mark_fine_coalitions) -> logits [B, n_coal, n_out] on the model's
        device, no autograd graph.  The game plays in one region (0 the promoter, 1 + j pCRE slot j); a player is a set of marks over a
        window of bins of the FINEST resolution, relative to the gene's `start` (attribution.fine_window_players: "windows", "cells" at
        `width` bins per window and `n_windows` windows, or (marks, (lo, hi)) pairs; at most 128).  `keep` as in mark_coalitions_wide.
        Column c is the inference forward with the marks of every ABSENT player, inside its window, scaled by `scale` in raw-signal
        space (0 erases; donor None) or taken from the donor (the forms of mark_donor_coalitions), at every resolution: a coarser bin
        the absent windows cover wholly follows mark_window_coalitions' rule, one they cover in part is recomputed from its finest
        children, weighted by their sample counts, as in perturbation_scan_fine; an element covered by several absent players changes
        once.  start: an int or B ints, the first finest genomic bin per gene; n_windows: default the windows that reach the end of
        the region from the smallest start; lengths, flip, return_feats ({binsize: [B, n_coal, n_bins, n_feats]}, the region's
        features that row (b, c) read; returned as (logits, feats)): as in perturbation_scan_fine.  One absent player gives the row of
        perturbation_scan_fine at that window, bit for bit; a window past the region's real bins changes nothing.  The packed forms of
        the first argument and the effect on a pending backward() are those of mark_coalitions."""
        from .attribution import mark_wide_words
        who = "mark_fine_window_coalitions"
        if keep is None:
            raise ValueError("mark_fine_window_coalitions: keep is required: the coalitions (bit p set: player p present)")
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        P, opts, _alive, _names = self._mark_fine_opts(who, bs.B, region, players, width, n_windows, start, lengths, scale, donor, flip)
        words = mark_wide_words(keep, P, who)
        feats = self._fine_feats(opts, bs.B, len(words)) if return_feats else None
        logits = self._mark_run_coalitions("cf_mark_fine_coalitions", bs, opts, words, book)
        return (logits, feats) if return_feats else logits

    @torch.no_grad()
    def mark_fine_window_shapley(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                 interaction_freq=None, region=0, players="windows", width=1, n_windows=None, start=0, lengths=None, scale=0.0,
                                 donor=None, flip=None, return_coalitions=False, return_feats=False):
        """Exact Shapley values of at most 16 fine window players (cf_mark_fine_shapley) -> (phi, info) with the keys of
        mark_window_shapley (info["feats"] with return_feats): which 200 bp of the peak carries the prediction?  Neighbouring fine windows
        share the credit here, where the leave-one-out perturbation_scan_fine scores redundant ones near zero.  Everything else as in
        mark_fine_window_coalitions; a null player (a window past the region's real bins, a dummy slot, a donor that agrees with the gene
        inside the window) has phi exactly 0."""
        who = "mark_fine_window_shapley"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        P, opts, _alive, names = self._mark_fine_opts(who, bs.B, region, players, width, n_windows, start, lengths, scale, donor, flip)
        if P > 16:
            raise ValueError("%s: %d players; the exact game takes 1..16: choose a larger width or mark_fine_window_shapley_sampled" % (who, P))
        feats = self._fine_feats(opts, bs.B, 1 << P) if return_feats else None
        phi, info = self._mark_run_shapley("cf_mark_fine_shapley", bs, opts, names, "erased" if donor is None else "donor", book, return_coalitions)
        if return_feats:
            info["feats"] = feats
        return phi, info

    @torch.no_grad()
    def mark_fine_window_shapley_interactions(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None,
                                              interaction_masks=None, interaction_freq=None, region=0, players="windows", width=1, n_windows=None,
                                              start=0, lengths=None, scale=0.0, donor=None, flip=None, index="sii", return_coalitions=False,
                                              return_feats=False):
        """Pairwise Shapley interaction indices of 2..16 fine window players (cf_mark_fine_shapley_interactions) -> (inter, info),
        tensors on the model's device, no autograd graph: which 200 bp stretches of the peak are redundant, which cooperate?  The 2^P
        coalitions run once, as in mark_fine_window_shapley:

          inter               [B, P, P, n_out], exactly symmetric.  Off the diagonal, with S over the coalitions that hold neither player,
                              I_ij = sum_S w(|S|) ((v(S + i + j) - v(S + j)) - (v(S + i) - v(S))): how much i's marginal contribution
                              changes with j present, averaged over every context -- negative for redundant players, positive for
                              cooperating ones, also where a third player hides the effect from the full-coalition *_epistasis.  index "sii"
                              (Shapley interaction index): w(s) = s! (P - s - 2)! / (P - 1)!, the diagonal is phi.  index "sti"
                              (Shapley-Taylor, order 2): w(s) = (2 / P) / C(P - 1, s), the diagonal is v({i}) - v(nobody), and the
                              diagonal plus the upper triangle sums to logits - erased.  A null player's row and column are exactly 0
          info["phi"]         [B, P, n_out]: the Shapley values of mark_fine_window_shapley on the same rows, bit for bit
          info["logits"]      [B, n_out]: the prediction;  info["erased"]  [B, n_out]: every player absent
          info["index"]       the index name;  info["delta"]  [B, n_out], "sti" only: the efficiency gap (rounding only)
          info["players"]     the players' names
          info["coalitions"]  [B, 2^P, n_out], with return_coalitions: the logits of every coalition, word m at column m

        SHAP's interaction values follow from the sii result: Phi_ij = I_ij / 2 off the diagonal and Phi_ii = phi_i - sum_{j != i} I_ij / 2.
        info["donor"] takes the place of info["erased"] with a donor; info["feats"] with return_feats.  Everything else as in
        mark_fine_window_shapley; a null player (a window past the region's real bins, a dummy slot, a donor that agrees with the gene
        inside the window) has its row and column exactly 0."""
        who = "mark_fine_window_shapley_interactions"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        P, opts, _alive, names = self._mark_fine_opts(who, bs.B, region, players, width, n_windows, start, lengths, scale, donor, flip)
        if P > 16:
            raise ValueError("%s: %d players; the exact game takes 2..16 and the index has no sampled estimator: choose a larger width" % (who, P))
        feats = self._fine_feats(opts, bs.B, 1 << P) if return_feats else None
        inter, info = self._mark_run_interactions("cf_mark_fine_shapley_interactions", bs, opts, names, "erased" if donor is None else "donor", book,
                                                  index, return_coalitions)
        if return_feats:
            info["feats"] = feats
        return inter, info

    @torch.no_grad()
    def mark_fine_window_shapley_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                                         interaction_freq=None, region=0, players="windows", width=1, n_windows=None, start=0, lengths=None,
                                         n_perm=64, seed=0, permutations=None, scale=0.0, donor=None, flip=None, return_rows=False,
                                         return_feats=False):
        """Permutation-sampled Shapley values of up to 128 fine window players (cf_mark_fine_shapley_sampled) -> (phi, info) with the
        keys, the row layout and the estimator of mark_shapley_sampled (info["feats"] with return_feats): which mark in which 200 bp?
        region, players, width, n_windows, start, lengths, scale, donor and flip as in mark_fine_window_coalitions; n_perm, seed and
        permutations as in mark_shapley_sampled.  A null player has phi and stderr exactly 0."""
        who = "mark_fine_window_shapley_sampled"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        P, opts, _alive, names = self._mark_fine_opts(who, bs.B, region, players, width, n_windows, start, lengths, scale, donor, flip)
        perms = self._permutations(who, P, n_perm, seed, permutations)
        feats = self._fine_feats(opts, bs.B, 2 + len(perms) * (P - 1)) if return_feats else None
        phi, info = self._mark_run_sampled("cf_mark_fine_shapley_sampled", bs, opts, names, perms, book, return_rows)
        if return_feats:
            info["feats"] = feats
        return phi, info

    @torch.no_grad()
    def mark_fine_window_shapley_interactions_sampled(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None,
                                                      interaction_masks=None, interaction_freq=None, region=0, players="windows", width=1,
                                                      n_windows=None, start=0, lengths=None, focal=None, index="sii", n_perm=64, seed=0,
                                                      permutations=None, scale=0.0, donor=None, flip=None, return_rows=False):
        """Permutation-sampled pairwise Shapley interaction indices of focal players among up to 128 fine window players
        (cf_mark_fine_shapley_interactions_sampled) -> (inter, info) with the keys, the row layout and the estimator of
        mark_shapley_interactions_sampled: which 200 bp stretches are redundant with the ones that carry the prediction?  region,
        players, width, n_windows, start, lengths, scale, donor and flip as in mark_fine_window_coalitions; focal, index, n_perm, seed
        and permutations as in mark_shapley_interactions_sampled.  The estimate is not symmetric; a null player has its row and column
        exactly 0."""
        who = "mark_fine_window_shapley_interactions_sampled"
        bs, _keep, book = self._attrib_call(who, (promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))
        P, opts, _alive, names = self._mark_fine_opts(who, bs.B, region, players, width, n_windows, start, lengths, scale, donor, flip)
        perms = self._permutations(who, P, n_perm, seed, permutations)
        return self._mark_run_pairs_sampled("cf_mark_fine_shapley_interactions_sampled", bs, opts, names, perms, focal, index, book, return_rows)

    def mark_fine_window_shapley_dataset(self, dataset, donor_dataset=None, genes=None, region="promoter", zoom=1, coarse_width=1, width=2,
                                         players="windows", n_perm=64, seed=0, scale=0.0, target=None, bsz=None, store=None, donor_store=None,
                                         interactions=None, dividends=False):
        """Shapley values of fine window players over the genes of a ChromoformerDataset, zooming from the coarse window game, against a
        donor cell type's dataset if one is given, windows in genomic coordinates (chromoformer_amd.attribution.mark_fine_window_shapley,
        a generator of per-gene dicts)."""
        from .attribution import mark_fine_window_shapley
        return mark_fine_window_shapley(self, dataset, donor_dataset, genes=genes, region=region, zoom=zoom, coarse_width=coarse_width, width=width,
                                        players=players, n_perm=n_perm, seed=seed, scale=scale, target=target, bsz=bsz, store=store,
                                        donor_store=donor_store, interactions=interactions, dividends=dividends)

    def raw_signal_gradients(self, dataset, genes=None, target=None, times_input=False, bsz=None):
        """Raw-signal saliency of the genes of a ChromoformerDataset: the gradient (or gradient x input) of logit column `target` with
        respect to the raw fp16 signals, per gene one track per histone mark for the promoter window and every pCRE, in genomic
        orientation (chromoformer_amd.attribution.raw_signal_gradients, a generator of per-gene dicts)."""
        from .attribution import raw_signal_gradients
        return raw_signal_gradients(self, dataset, genes=genes, target=target, times_input=times_input, bsz=bsz)

    def raw_integrated_gradients(self, dataset, genes=None, target=None, n_steps=50, method="gausslegendre", bsz=None, donor_dataset=None):
        """Integrated gradients of logit column `target` with respect to the raw fp16 signals of the genes of a ChromoformerDataset, from
        the zero signal along a * x: per gene one track per histone mark for the promoter window and every pCRE, in genomic
        orientation, summing to logits - baseline_logits up to the quadrature error.  donor_dataset: another cell type's dataset over
        the same regions; the baseline is then its signal xd and the path xd + a * (x - xd)
        (chromoformer_amd.attribution.raw_integrated_gradients, a generator of per-gene dicts)."""
        from .attribution import raw_integrated_gradients
        return raw_integrated_gradients(self, dataset, genes=genes, target=target, n_steps=n_steps, method=method, bsz=bsz,
                                        donor_dataset=donor_dataset)

    @torch.no_grad()
    def trunk_outputs(self, promoter_feats, promoter_pad_masks=None, pcre_feats=None, pcre_pad_masks=None, interaction_masks=None,
                      interaction_freq=None):
        """The trunk's output, the input of the Regulation stacks (cf_trunk_outputs) -> {binsize: [B, i_max + 1, d_emb]} on the model's
        device, no autograd graph: row 0 the promoter's centre-bin embedding, row 1 + j that of the promoter attending pCRE slot j.  For
        fixed Embedding + Pairwise weights it depends on the gene alone -- what engine.TrunkCache keeps for Trainer(freeze_trunk=True).
        The first argument may also be a packed batch (an engine.Slot or a pack_batch result), with nothing after it.  The pass
        overwrites the activations a grad-enabled model(...) keeps for its backward: such a pending backward() raises."""
        return dict(zip(self.binsizes, self._trunk_outputs((promoter_feats, promoter_pad_masks, pcre_feats, pcre_pad_masks, interaction_masks, interaction_freq))))

    def _trunk_outputs(self, batch, outs=None):
        """batch: the six arguments of trunk_outputs, or a batch struct."""
        bs, _keep, book = self._attrib_call("trunk_outputs", (batch, None) if isinstance(batch, _lib.cf_batch) else batch)
        if outs is None:
            outs = [torch.empty(bs.B, self.i_max + 1, self.d_emb, device=self._device) for _ in self.binsizes]      # (written in full by the library)
        ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        st = book()
        _lib.check(_lib.lib().cf_trunk_outputs(self._handle, C.byref(bs), ptrs, st), "cf_trunk_outputs")
        return outs

    def trunk_version(self):
        """Sum of the torch version counters of the trunk's parameters (what _sync_tiled sums over all of them): changes whenever one
        of them is written through torch."""
        return sum(p._version for n, p in self.named_parameters() if is_trunk_name(n))

    def embed_full(self, promoter_feats, promoter_pad_masks):
        """EmbeddingTransformer's first return value (net.py:57-59): {binsize: [B, 1, L, 128]}, the embedding of every
        promoter bin (all rows of every Embedding layer through the dense transformer layer; forward only)."""
        if self._handle is None:
            raise RuntimeError("call .cuda() first: the Chromoformer HIP path needs device buffers")
        bs = _lib.cf_batch()
        keep, B = [], None
        for r, b in enumerate(self.binsizes):
            L = self.n_bins[r]
            pf = promoter_feats[b].to(self._device, torch.float32).contiguous()
            B = pf.shape[0] if B is None else B
            if pf.numel() != B * L * self.n_feats:
                raise ValueError("promoter feature shape does not match the configuration at binsize %d" % b)
            m, ptr, stride = self._rows(promoter_pad_masks[b], L, B)
            keep += [pf, m]
            bs.promoter_feats[r], bs.promoter_mask_row[r], bs.promoter_mask_stride[r] = pf.data_ptr(), ptr, stride
            # cf_embed_full touches the promoter side only; the other pointers just have to be non-null
            bs.pcre_feats[r], bs.pcre_mask_row[r], bs.pcre_mask_stride[r], bs.interaction_mask[r] = pf.data_ptr(), ptr, stride, ptr
        bs.interaction_freq = keep[0].data_ptr()
        bs.B = B
        if B > self._max_batch:
            raise ValueError("batch of %d genes exceeds max_batch=%d given at construction" % (B, self._max_batch))
        outs = [torch.empty(B, 1, L, self.d_emb, device=self._device) for L in self.n_bins]
        ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        st = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(_lib.lib().cf_embed_full(self._handle, C.byref(bs), ptrs, st), "cf_embed_full")
        return {b: o for b, o in zip(self.binsizes, outs)}

    def forward_backward(self, packed, labels, loss_scale=1.0):
        """Fused forward + loss + backward.  Returns (logits, loss tensor on device)."""
        bs, _ = packed
        labels = labels.to(self._device)
        labels = labels.float().contiguous() if self.n_out == 1 else labels.long().contiguous()
        st = torch.cuda.current_stream(self._device).cuda_stream
        # head forward + loss + head backward at the tail of the Regulation forward launch where the library can (cf_forward_train),
        # else as one launch inside the cf_backward below; logits / loss are filled by whichever runs
        logits = torch.empty(bs.B, self.n_out, device=self._device)
        self._sync_tiled(st)
        _lib.check(_lib.lib().cf_forward_train(self._handle, C.byref(bs), logits.data_ptr(), labels.data_ptr(), float(loss_scale),
                                               self._loss_buf.data_ptr(), st), "cf_forward_train")
        _lib.check(_lib.lib().cf_backward(self._handle, C.byref(bs), labels.data_ptr(), float(loss_scale),
                                          self._loss_buf.data_ptr(), st), "cf_backward")
        self._grads_stale, self._grads_top = False, None      # (a full backward: every trainable gradient has just been written)
        return logits, self._loss_buf

    def adamw_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
        self._step += 1
        st = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(_lib.lib().cf_adamw_step(self._handle, float(lr), betas[0], betas[1], eps, weight_decay, self._step, st),
                   "cf_adamw_step")

    def active_grads(self):
        """The contiguous gradient range the optimiser / all-reduce operate on.  Raises after a step that never wrote it (the
        single-GPU Trainer applies AdamW in the epilogue of the gradient reductions and stores gradients only with
        keep_grads=True): stale values must not reach clip_grad_norm_ / logging / a custom all-reduce silently."""
        if getattr(self, "_grads_stale", False):
            raise RuntimeError("the gradient buffer was not written by the last step (Trainer(fuse_opt=True, keep_grads=False) "
                               "updates parameters inside the gradient reductions); construct the Trainer with keep_grads=True")
        top = getattr(self, "_grads_top", None)
        if top is not None:      # the last step ran on a frozen trunk: the Regulation + head range is all it wrote
            return top
        return self._gflat[: self._layout.n_active]

    def _mark_grads(self, stale, top=None):
        """Called by the Trainer after every step: `stale` = the step did not store its gradients; `top` = the step ran on a frozen
        trunk and wrote (at most) this range of the flat gradient buffer, the Regulation + head bucket."""
        if stale and not getattr(self, "_grads_stale", False):
            for p in self._named().values():      # `.grad` views of the flat buffer (loss.backward() publishes them) would read old values
                p.grad = None
        elif top is not None and getattr(self, "_grads_top", None) is None:
            for n, p in self._named().items():
                if is_trunk_name(n):
                    p.grad = None
        self._grads_stale = bool(stale)
        self._grads_top = top

    def train_step(self, packed, labels, lr, process_group=None, world_size=1):
        """zero_grad -> forward -> loss -> backward -> [all-reduce] -> AdamW (train.py:182-196)."""
        logits, loss = self.forward_backward(packed, labels, loss_scale=1.0 / world_size)
        if world_size > 1:
            torch.distributed.all_reduce(self.active_grads(), group=process_group)
        self.adamw_step(lr)
        return logits, loss

    def debug_buffer(self, name):
        n = C.c_longlong()
        _lib.check(_lib.lib().cf_debug_copy(self._handle, name.encode(), None, C.byref(n), None), "cf_debug_copy")
        out = torch.empty(n.value, device=self._device)
        st = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(_lib.lib().cf_debug_copy(self._handle, name.encode(), out.data_ptr(), C.byref(n), st), "cf_debug_copy")
        return out

    def launch_counts(self):
        f, b, o = C.c_int(), C.c_int(), C.c_int()
        _lib.check(_lib.lib().cf_launch_counts(self._handle, C.byref(f), C.byref(b), C.byref(o)), "cf_launch_counts")
        return f.value, b.value, o.value


class ChromoformerClassifier(ChromoformerBase):
    n_out = 2


class ChromoformerRegressor(ChromoformerBase):
    n_out = 1


_LEGACY_PREFIX = (("embed.", "embed"), ("pairwise_interaction.", "pw_int"), ("regulation.", "reg"))


class Chromoformer(ChromoformerClassifier):
    """The reference's original class (net.py:156-270): flat constructor arguments, a 16-positional-argument ``forward``
    (five tensors per resolution 2000 / 500 / 100, then the interaction frequencies) and modules named ``embed2000``,
    ``pw_int2000``, ``reg2000`` ... in its ``state_dict``.  Same construction order, so the same seed gives the same
    weights as ChromoformerClassifier (the reference's own smoke block checks that equality, net.py:431-568)."""

    def __init__(self, n_feats=7, embed_n_layers=1, embed_n_heads=2, embed_d_model=128, embed_d_ff=128, pw_int_n_layers=2,
                 pw_int_n_heads=2, pw_int_d_model=128, pw_int_d_ff=256, reg_n_layers=6, reg_n_heads=8, reg_d_model=256,
                 reg_d_ff=256, head_n_feats=128, seed=42, **kwargs):
        super().__init__(n_feats, embed_d_model, head_n_feats,
                         dict(n_layers=embed_n_layers, n_heads=embed_n_heads, d_model=embed_d_model, d_ff=embed_d_ff),
                         dict(n_layers=pw_int_n_layers, n_heads=pw_int_n_heads, d_model=pw_int_d_model, d_ff=pw_int_d_ff),
                         dict(n_layers=reg_n_layers, n_heads=reg_n_heads, d_model=reg_d_model, d_ff=reg_d_ff),
                         binsizes=(2000, 500, 100), seed=seed, **kwargs)

    def forward(self, x_p_2000, pad_mask_p_2000, x_pcre_2000, pad_mask_pcre_2000, interaction_mask_2000,
                x_p_500, pad_mask_p_500, x_pcre_500, pad_mask_pcre_500, interaction_mask_500,
                x_p_100, pad_mask_p_100, x_pcre_100, pad_mask_pcre_100, interaction_mask_100, interaction_freq):
        return super().forward({2000: x_p_2000, 500: x_p_500, 100: x_p_100},
                               {2000: pad_mask_p_2000, 500: pad_mask_p_500, 100: pad_mask_p_100},
                               {2000: x_pcre_2000, 500: x_pcre_500, 100: x_pcre_100},
                               {2000: pad_mask_pcre_2000, 500: pad_mask_pcre_500, 100: pad_mask_pcre_100},
                               {2000: interaction_mask_2000, 500: interaction_mask_500, 100: interaction_mask_100}, interaction_freq)

    @staticmethod
    def _legacy_key(k):
        for new, old in _LEGACY_PREFIX:
            if k.startswith(new):
                return old + k[len(new):]
        return k

    @staticmethod
    def _current_key(k):
        for new, old in _LEGACY_PREFIX:
            if k.startswith(old) and k[len(old):len(old) + 1].isdigit():
                return new + k[len(old):]
        return k

    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        return type(sd)((self._legacy_key(k), v) for k, v in sd.items())

    def load_state_dict(self, state_dict, strict=True):
        return super().load_state_dict(type(state_dict)((self._current_key(k), v) for k, v in state_dict.items()), strict=strict)
