"""The flat optimizer state between load_state_dict() and the first step(), on the CPU: optim.AdamW and optim.SGD keep the loaded `pfst_flat`
entries in `_pending_flat` until an arena steps, and state_dict() has to return them meanwhile -- a checkpoint written after a resume and
before a step would otherwise drop the moments, the step count and the momentum buffer.  No arena and no launch is needed: a state with
`pfst_flat` entries is loaded into an optimizer over a CPU parameter and read back.  (tests/test_optimizer_edges_gpu.py steps afterwards.)"""
import pytest
import torch


def _entries(kind, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == 'AdamW':
        return [dict(m=torch.randn(8, generator=gen), v=torch.rand(8, generator=gen), step=3 + i) for i in range(2)]
    return [dict(buf=torch.randn(8, generator=gen), stepped=True), dict(buf=None, stepped=False)]


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.is_tensor(b[k]) and torch.equal(a[k], b[k]), k
        else:
            assert a[k] is b[k] or (a[k] == b[k] and type(a[k]) is type(b[k])), k


@pytest.mark.parametrize('kind', ['AdamW', 'SGD'])
def test_state_dict_returns_the_pending_flat_entries(kind):
    from pfst_amd import optim
    make = (lambda ps: optim.AdamW(ps, lr=6e-5)) if kind == 'AdamW' else (lambda ps: optim.SGD(ps, lr=0.01, momentum=0.9))
    opt = make([torch.nn.Parameter(torch.zeros(5))])
    sd = opt.state_dict()
    assert sd['pfst_flat'] == []
    loaded = _entries(kind, 7)
    sd['pfst_flat'] = loaded
    opt.load_state_dict(sd)
    assert len(sd['pfst_flat']) == 2 and sd['pfst_flat'] is loaded               # the caller's dict is left as it was
    for _ in range(2):                                                            # reading it back does not consume it
        back = opt.state_dict()['pfst_flat']
        assert len(back) == 2
        for a, b in zip(back, _entries(kind, 7)):
            _same(a, b)
    # ... and the round trip goes on through a second optimizer that never stepped either
    opt2 = make([torch.nn.Parameter(torch.zeros(5))])
    opt2.load_state_dict(opt.state_dict())
    for a, b in zip(opt2.state_dict()['pfst_flat'], _entries(kind, 7)):
        _same(a, b)
    assert len(opt.state_dict()['pfst_flat']) == 2                               # loading elsewhere took nothing from the first


def test_optimizer_dict_returns_the_pending_entries_of_every_member():
    from pfst_amd import optim
    od = optim.OptimizerDict(a=optim.AdamW([torch.nn.Parameter(torch.zeros(3))]), b=optim.AdamW([torch.nn.Parameter(torch.zeros(4))]))
    sd = od.state_dict()
    sd['a']['pfst_flat'], sd['b']['pfst_flat'] = _entries('AdamW', 1)[:1], _entries('AdamW', 2)
    od.load_state_dict(sd)
    back = od.state_dict()
    assert [len(back[k]['pfst_flat']) for k in ('a', 'b')] == [1, 2]
    _same(back['a']['pfst_flat'][0], _entries('AdamW', 1)[0])
    _same(back['b']['pfst_flat'][1], _entries('AdamW', 2)[1])
