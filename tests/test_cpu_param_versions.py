"""engine._weights_token: what SurvivalEngine.sync_packs compares to decide whether the derived conv2 packs are stale.  The parameters are
attached to the engine's flat buffer as `p.data = view_of_flat` (SurvivalEngine._flatten), which gives each parameter a version counter
of its own: every in-place change of a PARAMETER must move the token, a write to the flat buffer must move it, reads must not, and a write
through `p.data` cannot (the limit sync_packs' docstring states; `sync_packs(force=True)` covers it).  Host logic only: runs on the CPU."""
import pytest
import torch
import torch.nn as nn


def _attached(seed=0):
    """A tiny module whose parameters are views of one flat buffer, attached exactly as SurvivalEngine._flatten does (one of them a strided
    view like the packed conv2 weights) -> (module, params, flat)."""
    torch.manual_seed(seed)
    m = nn.Sequential(nn.Linear(6, 4), nn.Linear(4, 3))
    params = list(m.parameters())
    flat = torch.zeros(sum(p.numel() for p in params))
    o = 0
    with torch.no_grad():
        for i, p in enumerate(params):
            if i == 0:      # [4, 6] stored as [6][4]: a strided view with the parameter's shape
                v = flat.as_strided((4, 6), (1, 4), o)
            else:
                v = flat[o:o + p.numel()].view_as(p)
            v.copy_(p.data)
            p.data = v
            o += p.numel()
    return m, params, flat


def _tok(params, flat):
    from multimodal_survival_prediction_amd.engine import _weights_token
    return _weights_token(params, flat)


def _set_grads(params):
    for p in params:
        p.grad = torch.ones_like(p)


def _mul(m, params, flat):
    with torch.no_grad():
        params[0].mul_(-1.5)


def _copy(m, params, flat):
    with torch.no_grad():
        params[2].copy_(torch.randn_like(params[2]))


def _load(m, params, flat):
    m.load_state_dict({k: torch.randn_like(v) for k, v in m.state_dict().items()})


def _sgd(m, params, flat):
    _set_grads(params)
    torch.optim.SGD(params, lr=0.1).step()


def _adam(foreach):
    def step(m, params, flat):
        _set_grads(params)
        torch.optim.Adam(params, lr=0.1, foreach=foreach).step()
    return step


def _flat_copy(m, params, flat):
    flat.copy_(torch.randn_like(flat))


CHANGES = {"mul_": _mul, "copy_": _copy, "load_state_dict": _load, "sgd_step": _sgd, "adam_step_foreach": _adam(True),
           "adam_step_single": _adam(False), "flat_copy_": _flat_copy}


@pytest.mark.parametrize("kind", sorted(CHANGES))
def test_token_moves_with_every_detectable_change(kind):
    m, params, flat = _attached()
    before_vals = flat.clone()
    t0 = _tok(params, flat)
    assert _tok(params, flat) == t0                       # reading the token does not move it
    CHANGES[kind](m, params, flat)
    assert not torch.equal(flat, before_vals)             # (the change did reach the flat buffer: the views are still attached)
    assert _tok(params, flat) != t0


def test_token_is_still_for_reads():
    m, params, flat = _attached()
    _set_grads(params)
    t0 = _tok(params, flat)
    s = sum(float(p.detach().sum()) for p in params) + float(m(torch.ones(2, 6)).sum().detach())    # reads, an autograd forward included
    sd = m.state_dict()
    _ = {k: v.clone() for k, v in sd.items()}
    m.zero_grad()
    m.zero_grad(set_to_none=True)
    _set_grads(params)
    assert s == s and _tok(params, flat) == t0


def test_data_write_is_invisible():
    """The stated limit: `p.data` is a fresh alias without the parameter's version counter, and the flat buffer's counter belongs to
    another tensor -- a write through it moves the numbers and no counter."""
    m, params, flat = _attached()
    before_vals = flat.clone()
    t0 = _tok(params, flat)
    params[0].data.mul_(-1.5)
    assert not torch.equal(flat, before_vals)
    assert _tok(params, flat) == t0


def test_token_watches_only_the_given_parameters():
    """The engine passes its 58 conv2 parameters: a change of another parameter of the flat buffer needs no re-pack and moves nothing."""
    m, params, flat = _attached()
    t0 = _tok(params[:1], flat)
    with torch.no_grad():
        params[1].mul_(2.0)
    assert _tok(params[:1], flat) == t0
    with torch.no_grad():
        params[0].mul_(2.0)
    assert _tok(params[:1], flat) != t0
