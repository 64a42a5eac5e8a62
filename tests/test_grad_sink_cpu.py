"""The gradient-sink protocol between GeoTrainer and an op that writes
its weight gradient in place (geomx_amd/gradsink.py), without the
extension: a test-double autograd.Function fills the sink's view in
plain torch.

Every case runs the same model twice, with sinks attached and with
`grad_sinks=False` (every span cleared by zero_grad() and filled by
autograd's accumulation), and asks for identical buckets and
parameters: a sink may remove passes, never change a number."""

import torch
import torch.nn.functional as F

from dist_helpers import run_dist

from geomx_amd import Config, gradsink
from geomx_amd.kvstore.optimizer import OptimizerSpec, ServerOptimizer
from geomx_amd.parallel import GeoTrainer
from geomx_amd.topology import init_topology


class _SinkLinearFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        ctx.sink = gradsink.sink_of(weight)
        return x @ weight.detach().t()

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        gw = dy.t() @ x
        dst = None if ctx.sink is None else ctx.sink.take()
        if dst is not None:
            dst.copy_(gw)
            gw = dst
        return dy @ weight, gw


class SinkLinear(torch.nn.Linear):
    """nn.Linear (no bias) whose backward can write the weight gradient
    into a sink; `native = False` takes the plain autograd route."""
    native = True

    def __init__(self, i, o):
        super().__init__(i, o, bias=False)

    def grad_sink_parameters(self):
        return (self.weight,)

    def forward(self, x):
        if self.native:
            return _SinkLinearFn.apply(x, self.weight)
        return F.linear(x, self.weight)


def _model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(
        torch.nn.Linear(6, 5), torch.nn.ReLU(), SinkLinear(5, 4),
        torch.nn.ReLU(), torch.nn.Linear(4, 3))


def _data(seed, n=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 6, generator=g), torch.randint(0, 3, (n,),
                                                         generator=g)


def _trainer(model, sinks, lr=0.05):
    cfg = Config.from_env(backend="gloo", device="cpu", bucket_mb=1)
    topo = init_topology(1, None, None, "cpu")   # single-process world
    return GeoTrainer(model, cfg, topo,
                      OptimizerSpec(name="sgd_mom", lr=lr, momentum=0.9),
                      grad_sinks=sinks)


def _loss_plain(model, x, y):
    return F.cross_entropy(model(x), y)


def _span(tr, p):
    b, i = tr.param_bucket[p]
    return b.views[i]


def _run(sinks, loss_fn=_loss_plain, steps=2, backwards=1, prepare=None,
         zero="trainer"):
    """`steps` training steps; returns (buckets before each update,
    final parameters)."""
    model = _model()
    if prepare is not None:
        prepare(model)
    tr = _trainer(model, sinks)
    assert (len(tr.sinks) == 1) == sinks
    flats = []
    for s in range(steps):
        if zero == "trainer":
            tr.zero_grad()
        else:
            model.zero_grad()          # set_to_none: drops every view
        for k in range(backwards):
            x, y = _data(10 * s + k)
            loss_fn(model, x, y).backward()
        tr.allreduce_grads()
        flats.append([b.flat.clone() for b in tr.buckets])
        for p in model.parameters():   # the documented contract
            assert p.grad.data_ptr() == _span(tr, p).data_ptr()
        tr.update()
    return flats, [p.detach().clone() for p in model.parameters()]


def _same(a, b):
    fa, pa = a
    fb, pb = b
    for sa, sb in zip(fa, fb):
        for x, y in zip(sa, sb):
            assert torch.equal(x, y)
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)


def test_adoption_without_copy():
    model = _model()
    w = model[2].weight
    seen = []
    # registered before the trainer's hook, so it sees what autograd
    # installed, before any repair
    w.register_post_accumulate_grad_hook(
        lambda p: seen.append(p.grad.data_ptr()))
    tr = _trainer(model, True)
    sink = tr.sinks[w]
    for s in range(2):
        tr.zero_grad()
        assert w.grad is None and sink.armed
        x, y = _data(s)
        _loss_plain(model, x, y).backward()
        assert not sink.armed
        assert seen[-1] == sink.data_ptr() == _span(tr, w).data_ptr()
        assert w.grad.data_ptr() == sink.data_ptr()
        assert w.grad.shape == w.shape and w.grad.stride() == w.stride()
        # the gradient itself, against plain autograd on the same graph
        model[2].native = False
        gref, = torch.autograd.grad(_loss_plain(model, x, y), w)
        model[2].native = True
        assert torch.allclose(w.grad, gref, atol=1e-6)
        tr.step()


def test_take_is_once_per_zero_grad_and_fresh():
    model = _model()
    tr = _trainer(model, True)
    sink = tr.sinks[model[2].weight]
    assert sink.take() is None            # not armed before zero_grad()
    tr.zero_grad()
    v = sink.take()
    assert v is not None and v.data_ptr() == sink.data_ptr()
    assert sink.take() is None
    tr.zero_grad()
    v2 = sink.take()
    assert v2 is not None and v2 is not v


def test_matches_fill_and_add_over_steps():
    _same(_run(True, steps=3), _run(False, steps=3))


def test_second_backward_before_step_sums():
    a = _run(True, backwards=2)
    _same(a, _run(False, backwards=2))
    # and it IS the sum: one backward of each batch alone
    model = _model()
    w = model[2].weight
    gs = []
    for k in range(2):
        x, y = _data(k)
        gs.append(torch.autograd.grad(_loss_plain(model, x, y), w)[0])
    tr = _trainer(_model(), True)
    span = _span(tr, tr.model[2].weight)
    tr.zero_grad()
    for k in range(2):
        x, y = _data(k)
        _loss_plain(tr.model, x, y).backward()
    assert torch.allclose(span, gs[0] + gs[1], atol=1e-6)


def _run_seq(sinks, seq, steps=2):
    """Like _run, with the step's backwards (and its zero_grad) made by
    `seq(model, tr, s)`."""
    model = _model()
    tr = _trainer(model, sinks)
    flats = []
    for s in range(steps):
        seq(model, tr, s)
        tr.allreduce_grads()
        flats.append([b.flat.clone() for b in tr.buckets])
        for p in model.parameters():
            assert p.grad.data_ptr() == _span(tr, p).data_ptr()
        tr.update()
    return flats, [p.detach().clone() for p in model.parameters()]


def _seq_reg_first(model, tr, s):
    # a regulariser's backward of its own BEFORE the main one: the weight
    # gets its first gradient by a route that never sees the sink
    tr.zero_grad()
    (0.1 * model[2].weight.pow(2).sum()).backward()
    x, y = _data(30 + s)
    _loss_plain(model, x, y).backward()


def test_other_route_first_then_sink_route():
    """Once p.grad is set, by whatever route, the sink is spent: the
    native backward that follows must add to the span, not overwrite
    it and have autograd add the span to itself."""
    a = _run_seq(True, _seq_reg_first)
    _same(a, _run_seq(False, _seq_reg_first))
    # and the span IS the sum of the two gradients
    model = _model()
    tr = _trainer(model, True)
    w = model[2].weight
    _seq_reg_first(model, tr, 0)
    x, y = _data(30)
    model[2].native = False
    gref, = torch.autograd.grad(
        _loss_plain(model, x, y) + 0.1 * w.pow(2).sum(), w)
    assert torch.allclose(_span(tr, w), gref, atol=1e-6)
    assert not tr.sinks[w].armed


def _seq_mixed_routes(model, tr, s):
    # gradient accumulation: first micro-batch through the fallback
    # route, second through the native one
    tr.zero_grad()
    for k, native in enumerate((False, True)):
        model[2].native = native
        x, y = _data(40 + 2 * s + k)
        _loss_plain(model, x, y).backward()


def test_fallback_micro_batch_then_native_micro_batch():
    a = _run_seq(True, _seq_mixed_routes)
    _same(a, _run_seq(False, _seq_mixed_routes))
    model = _model()
    tr = _trainer(model, True)
    w = model[2].weight
    _seq_mixed_routes(model, tr, 0)
    model[2].native = False
    gs = [torch.autograd.grad(_loss_plain(model, *_data(40 + k)), w)[0]
          for k in range(2)]
    assert torch.allclose(_span(tr, w), gs[0] + gs[1], atol=1e-6)


def _seq_skip_then_backward_without_zero_grad(model, tr, s):
    if s == 0:
        # a step in which the sink parameter gets no gradient
        tr.zero_grad()
        x, y = _data(50)
        _loss_skip_sink(model, x, y).backward()
    else:
        # and a backward without a zero_grad() in between: p.grad is
        # the (settled) span, the sink must not hand it out
        x, y = _data(51)
        _loss_plain(model, x, y).backward()


def test_settled_step_then_backward_without_zero_grad():
    a = _run_seq(True, _seq_skip_then_backward_without_zero_grad)
    _same(a, _run_seq(False, _seq_skip_then_backward_without_zero_grad))


def test_take_refuses_while_grad_is_set():
    model = _model()
    tr = _trainer(model, True)
    w = model[2].weight
    sink = tr.sinks[w]
    tr.zero_grad()
    w.grad = torch.ones_like(w)           # set behind the trainer's back
    assert sink.take() is None and not sink.armed
    w.grad = None
    assert sink.take() is None            # spent until the next zero_grad()
    tr.zero_grad()
    assert sink.take() is not None


def _loss_twice(model, x, y):
    h = F.relu(model[0](x))
    h = F.relu(model[2](h))
    # the sink module a second time, on another input
    h = h + F.relu(model[2](h.detach().roll(1, 0) @ torch.ones(4, 5)))
    return F.cross_entropy(model[4](h), y)


def test_module_used_twice_sums_both():
    _same(_run(True, _loss_twice), _run(False, _loss_twice))
    model = _model()
    tr = _trainer(model, True)
    w = model[2].weight
    x, y = _data(3)
    tr.zero_grad()
    _loss_twice(model, x, y).backward()
    model[2].native = False
    gref, = torch.autograd.grad(_loss_twice(model, x, y), w)
    assert torch.allclose(_span(tr, w), gref, atol=1e-6)
    assert w.grad.data_ptr() == _span(tr, w).data_ptr()


def _loss_reg(model, x, y):
    return _loss_plain(model, x, y) + 0.1 * model[2].weight.pow(2).sum()


def test_weight_also_feeds_a_loss_term():
    _same(_run(True, _loss_reg), _run(False, _loss_reg))
    model = _model()
    tr = _trainer(model, True)
    w = model[2].weight
    x, y = _data(4)
    tr.zero_grad()
    _loss_reg(model, x, y).backward()
    model[2].native = False
    gref, = torch.autograd.grad(_loss_reg(model, x, y), w)
    assert torch.allclose(_span(tr, w), gref, atol=1e-6)
    assert w.grad.data_ptr() == _span(tr, w).data_ptr()


def _non_native(model):
    model[2].native = False


def test_non_sink_route_lands_in_bucket():
    a = _run(True, prepare=_non_native)
    _same(a, _run(False, prepare=_non_native))
    # the same numbers as the sink route gives: one gradient, two ways
    b = _run(True)
    for sa, sb in zip(a[0], b[0]):
        for x, y in zip(sa, sb):
            assert torch.allclose(x, y, atol=1e-6)


def _loss_skip_sink(model, x, y):
    h = F.relu(model[0](x))
    return F.cross_entropy(model[4](h[:, :4]), y)


def test_sink_parameter_without_gradient_contributes_zero():
    _same(_run(True, _loss_skip_sink), _run(False, _loss_skip_sink))
    model = _model()
    tr = _trainer(model, True)
    w = model[2].weight
    w0 = w.detach().clone()
    _span(tr, w).fill_(7.0)               # a stale gradient in the span
    tr.zero_grad()
    x, y = _data(5)
    _loss_skip_sink(model, x, y).backward()
    assert w.grad is None
    tr.allreduce_grads()
    assert w.grad.data_ptr() == _span(tr, w).data_ptr()
    assert torch.equal(_span(tr, w), torch.zeros_like(w))
    tr.update()
    assert torch.equal(w.detach(), w0)


def test_plain_model_zero_grad_still_updates_right():
    _same(_run(True, zero="model"), _run(True))
    _same(_run(False, zero="model"), _run(True))


def test_zero_grad_clears_only_ordinary_spans():
    model = _model()
    tr = _trainer(model, True)
    assert len(tr.buckets) == 1           # sink span between ordinary ones
    b = tr.buckets[0]
    w = model[2].weight
    at = [i for i, p in enumerate(b.params) if p is w]
    assert at and at[0] not in (0, len(b.params) - 1)
    b.flat.fill_(3.0)
    tr.zero_grad()
    keep = torch.zeros_like(b.flat, dtype=torch.bool)
    off = _span(tr, w).storage_offset()
    keep[off:off + w.numel()] = True
    assert torch.equal(b.flat[keep], torch.full((w.numel(),), 3.0))
    assert torch.equal(b.flat[~keep], torch.zeros(int((~keep).sum())))
    # without sinks the whole bucket is cleared, in one range
    tr2 = _trainer(_model(), False)
    tr2.buckets[0].flat.fill_(3.0)
    tr2.zero_grad()
    assert len(tr2.buckets[0].clear) == 1
    assert not tr2.buckets[0].flat.any()


def _ws2(rank, world):
    cfg = Config.from_env(num_parties=1, backend="gloo", device="cpu",
                          bucket_mb=1)
    topo = init_topology(cfg.num_parties, cfg.party_sizes, "gloo", "cpu")
    model = _model()
    tr = GeoTrainer(model, cfg, topo,
                    OptimizerSpec(name="sgd_mom", lr=0.05, momentum=0.9))
    w = model[2].weight
    # single-process reference on the combined batch, plain autograd
    ref_model = _model()
    ref_model[2].native = False
    ref = ServerOptimizer(OptimizerSpec(name="sgd_mom", lr=0.05,
                                        momentum=0.9))
    for s in range(3):
        x, y = _data(20 + s, n=4 * world)
        tr.zero_grad()
        assert w.grad is None
        _loss_plain(model, x[rank * 4:(rank + 1) * 4],
                    y[rank * 4:(rank + 1) * 4]).backward()
        # in the bucket when the hook fired
        assert w.grad.data_ptr() == _span(tr, w).data_ptr()
        tr.step()
        ref_model.zero_grad()
        _loss_plain(ref_model, x, y).backward()
        for i, p in enumerate(ref_model.parameters()):
            ref.update(i, p.data.reshape(-1), p.grad.reshape(-1).clone())
    for p, q in zip(model.parameters(), ref_model.parameters()):
        assert torch.allclose(p, q, atol=1e-5), (rank, (p - q).abs().max())


def test_ws2_matches_single_process():
    run_dist(2, _ws2)
