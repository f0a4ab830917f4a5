"""A second cf_bind on a live handle.  The library resolves every parameter reference once, at cf_bind; what that can break is
binding again: a pointer left over from the first bind would read the old parameter buffer or write the old gradient buffer.

Referee: a fresh model loaded with the same parameter values.  The same kernels in the same order give the same bits (the suite relies
on that for its eager-versus-graph comparisons), so every comparison here is torch.equal.  Two modes: the default configuration as it
ships (fused trunk + fused Regulation: device tables built at bind) and CF_TRUNK=0 + CF_REG_FUSED=0 (the stand-alone kernels, whose
launch arguments are filled from the references at every call)."""
import ctypes as C

import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests.helpers import build_model

pytestmark = pytest.mark.gpu
B = 2
MODES = {"fused": {}, "standalone": {"CF_TRUNK": "0", "CF_REG_FUSED": "0"}}


def _lib():
    from chromoformer_amd import _lib as L
    return L


def _bind(model, params, grads=None, m=None, v=None):
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    _lib().check(_lib().lib().cf_bind(model._handle, ptr(params), ptr(grads), ptr(m), ptr(v)), "cf_bind")


def _forward(model, bs, save):
    logits = torch.full((B, model.n_out), float("nan"), device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    _lib().check(_lib().lib().cf_forward(model._handle, C.byref(bs), logits.data_ptr(), save, st), "cf_forward")
    return logits


def _backward_rc(model, bs, labels, loss):
    st = torch.cuda.current_stream().cuda_stream
    return _lib().lib().cf_backward(model._handle, C.byref(bs), labels.data_ptr(), 1.0, loss.data_ptr(), st)


def _forward_backward(model, bs, labels):
    """Forward with save, then backward with the fused loss -> (logits, loss)."""
    loss = torch.full((1,), float("nan"), device="cuda:0")
    logits = _forward(model, bs, 1)
    _lib().check(_backward_rc(model, bs, labels, loss), "cf_backward")
    torch.cuda.synchronize()
    return logits, loss


class _Rebound:
    """Model A after one step on its own buffers, the new flat buffers, and the referee B loaded with the new parameter values."""

    def __init__(self, mode, monkeypatch):
        for k, v in MODES[mode].items():      # (read when a model is constructed / bound)
            monkeypatch.setenv(k, v)
        batch = orc.synthetic_batch(B, seed=17, regime="realistic")
        self.labels = batch["label"].long().cuda(0).contiguous()
        self.a = build_model(None, False, B)
        self.packed = self.a.pack_batch(batch)      # (device pointers only: the same batch serves both handles)
        self.bs = self.packed[0]
        self.a.forward_backward(self.packed, batch["label"])
        torch.cuda.synchronize()
        g = torch.Generator().manual_seed(23)
        self.params = (self.a._flat + 0.05 * torch.randn(self.a._flat.shape, generator=g).cuda(0)).contiguous()
        self.grads, self.m, self.v = (torch.zeros_like(self.params) for _ in range(3))
        self.b = build_model(None, False, B)
        with torch.no_grad():
            self.b._flat.copy_(self.params)
        self.b.params_changed()

    def poison(self):
        """A's first parameter buffer becomes NaN; -> a snapshot of its first gradient buffer."""
        with torch.no_grad():
            self.a._flat.fill_(float("nan"))
        torch.cuda.synchronize()
        return self.a._gflat.clone()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_second_bind_reads_and_writes_only_the_new_buffers(mode, monkeypatch):
    s = _Rebound(mode, monkeypatch)
    assert bool(_lib().lib().cf_head_rides(s.a._handle)) == (mode == "fused")
    _bind(s.a, s.params, s.grads, s.m, s.v)
    old_grads = s.poison()
    logits_a, loss_a = _forward_backward(s.a, s.bs, s.labels)
    logits_b, loss_b = _forward_backward(s.b, s.bs, s.labels)
    assert torch.equal(logits_a, logits_b) and torch.equal(loss_a, loss_b)
    assert torch.equal(s.grads, s.b._gflat)
    assert torch.equal(s.a._gflat, old_grads)
    assert not torch.isnan(logits_a).any() and not torch.isnan(loss_a).any() and not torch.isnan(s.grads).any()
    assert s.grads.abs().max().item() > 0.0


@pytest.mark.parametrize("mode", sorted(MODES))
def test_training_step_calls_on_the_rebound_handle(mode, monkeypatch):
    """The calls of the shipped step, cf_forward_train + cf_backward: in fused mode the head rides in the Regulation launches (its
    weights come from the references of the second bind), in stand-alone mode it is left to the backward call."""
    s = _Rebound(mode, monkeypatch)
    _bind(s.a, s.params, s.grads, s.m, s.v)
    old_grads = s.poison()
    labels = s.labels.cpu()
    logits_a, loss_a = s.a.forward_backward(s.packed, labels)
    torch.cuda.synchronize()
    logits_a, loss_a = logits_a.clone(), loss_a.clone()
    logits_b, loss_b = s.b.forward_backward(s.packed, labels)
    torch.cuda.synchronize()
    assert torch.equal(logits_a, logits_b) and torch.equal(loss_a, loss_b)
    assert torch.equal(s.grads, s.b._gflat)
    assert torch.equal(s.a._gflat, old_grads)
    assert not torch.isnan(logits_a).any() and not torch.isnan(loss_a).any() and not torch.isnan(s.grads).any()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_bind_without_gradient_buffers_then_with_them_again(mode, monkeypatch):
    s = _Rebound(mode, monkeypatch)
    _bind(s.a, s.params)
    old_grads = s.poison()
    logits_a, logits_b = _forward(s.a, s.bs, 0), _forward(s.b, s.bs, 0)
    torch.cuda.synchronize()
    assert torch.equal(logits_a, logits_b) and not torch.isnan(logits_a).any()
    # no gradient buffer: a saving forward is still legal, the backward is refused by name
    _forward(s.a, s.bs, 1)
    loss = torch.zeros(1, device="cuda:0")
    assert _backward_rc(s.a, s.bs, s.labels, loss) != 0
    assert "no gradient buffer bound" in _lib().lib().cf_last_error().decode()
    _bind(s.a, s.params, s.grads, s.m, s.v)
    logits_a, loss_a = _forward_backward(s.a, s.bs, s.labels)
    logits_b, loss_b = _forward_backward(s.b, s.bs, s.labels)
    assert torch.equal(logits_a, logits_b) and torch.equal(loss_a, loss_b)
    assert torch.equal(s.grads, s.b._gflat) and not torch.isnan(s.grads).any()
    assert torch.equal(s.a._gflat, old_grads)
