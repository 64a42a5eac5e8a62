"""Gradient-sink offers of the conv stages, the first dense layer and the
classifier tail, and what GeoTrainer.zero_grad() still clears once every
parameter of a bucket has a sink (CPU: the sinks stay unused there and
every gradient reaches its span through the trainer's hook)."""

import pytest
import torch
import torch.nn.functional as F

from geomx_amd import Config
from geomx_amd.kvstore.optimizer import OptimizerSpec
from geomx_amd.models import create_model
from geomx_amd.ops.conv import GeoConv5, GeoConv5Pool
from geomx_amd.ops.fc import GeoFlattenLinear, mlp_tail, tail_route
from geomx_amd.parallel import GeoTrainer
from geomx_amd.topology import init_topology


def _ids(ps):
    return [id(p) for p in ps]


def test_offers():
    c = GeoConv5Pool(3, 16)
    assert _ids(c.grad_sink_parameters()) == _ids((c.weight, c.bias))
    c = GeoConv5(16, 32, bias=False)
    assert _ids(c.grad_sink_parameters()) == _ids((c.weight,))
    f = GeoFlattenLinear(64, 8)
    assert _ids(f.grad_sink_parameters()) == _ids((f.weight, f.bias))
    f = GeoFlattenLinear(64, 8, bias=False)
    assert _ids(f.grad_sink_parameters()) == _ids((f.weight,))
    m = create_model("geomx_cnn", image_size=20)
    cl = m.classifier
    assert _ids(m.grad_sink_parameters()) == _ids(
        (cl[3].weight, cl[3].bias, cl[5].weight, cl[5].bias))
    assert sorted(m.state_dict()) == sorted(
        ["features.0.weight", "features.0.bias", "features.1.weight",
         "features.1.bias", "classifier.1.weight", "classifier.1.bias",
         "classifier.3.weight", "classifier.3.bias", "classifier.5.weight",
         "classifier.5.bias"])


def test_tail_is_the_eager_chain_off_the_gpu():
    m = create_model("geomx_cnn", image_size=20)
    x = torch.randn(4, 256)
    cl = m.classifier
    assert not tail_route(x, cl[3], cl[5])
    want = cl[5](F.relu(cl[3](F.relu(x))))
    assert torch.equal(mlp_tail(x, cl[3], cl[5]), want)
    img = torch.randn(2, 3, 20, 20)
    assert torch.equal(m(img), cl(m.features(img)))


def _trainer(model, sinks=True, **cfg):
    c = Config.from_env(backend="gloo", device="cpu", **cfg)
    topo = init_topology(1, None, None, "cpu")
    return GeoTrainer(model, c, topo,
                      OptimizerSpec(name="sgd_mom", lr=0.05, momentum=0.9),
                      grad_sinks=sinks)


def _padded(tr):
    """Mask of the alignment padding of every bucket."""
    out = []
    for b in tr.buckets:
        pad = torch.ones(b.flat.numel(), dtype=torch.bool)
        for v in b.views:
            o = v.storage_offset()
            pad[o:o + v.numel()] = False
        out.append(pad)
    return out


def test_clear_ranges_when_every_parameter_has_a_sink():
    tr = _trainer(create_model("geomx_cnn", image_size=20))
    assert len(tr.sinks) == 10
    pads = _padded(tr)
    assert any(bool(p.any()) for p in pads)      # there is padding
    for b in tr.buckets:
        assert b.clear == [] and b.gaps == []    # and nothing to fill
    # a DGT wire can write the padding: the gaps are kept, as ranges of
    # padding alone that cover all of it, outside `clear`
    tr = _trainer(create_model("geomx_cnn", image_size=20),
                  compression="dgt")
    for b, pad in zip(tr.buckets, _padded(tr)):
        assert b.clear == []
        seen = torch.zeros_like(pad)
        for r in b.gaps:
            o = r.storage_offset() - b.flat.storage_offset()
            assert bool(pad[o:o + r.numel()].all())
            seen[o:o + r.numel()] = True
        assert torch.equal(seen, pad)
        b.flat.fill_(3.0)
    tr.zero_grad()
    for b, pad in zip(tr.buckets, _padded(tr)):
        assert not bool(b.flat[pad].any())
        assert bool((b.flat[~pad] == 3.0).all())  # spans: the backward's


def test_mixed_bucket_and_no_sinks_keep_the_parent_ranges():
    # without sinks: the whole bucket, one range, whatever the wire
    for comp in (None, "dgt"):
        tr = _trainer(create_model("geomx_cnn", image_size=20), sinks=False,
                      compression=comp)
        for b in tr.buckets:
            assert len(b.clear) == 1 and b.gaps == []
            assert b.clear[0].numel() == b.flat.numel()

    # an ordinary parameter between sink spans: its run is cleared with
    # the padding around it, the pad-only run between two sinks is not
    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = GeoFlattenLinear(8, 3)          # sinks, 24 + 3
            self.b = torch.nn.Linear(3, 3)           # ordinary
            self.c = GeoFlattenLinear(3, 2)          # sinks

        def forward(self, x):
            return self.c(self.b(self.a(x)))

    tr = _trainer(M())
    b, = tr.buckets
    # reverse order: c.bias, c.weight | b.bias, b.weight | a.bias, a.weight
    offs = [v.storage_offset() for v in b.views]
    assert offs == [0, 64, 128, 192, 256, 320]
    rng = [(r.storage_offset(), r.numel()) for r in b.clear]
    assert rng == [(64 + 6, 256 - 70)] and b.gaps == []
    b.flat.fill_(3.0)
    tr.zero_grad()
    assert not bool(b.flat[70:256].any())
    assert bool((b.flat[:70] == 3.0).all()) and bool((b.flat[256:] == 3.0).all())


@pytest.mark.parametrize("steps", [1, 3])
def test_training_is_the_same_with_and_without_sinks(steps):
    def run(sinks):
        torch.manual_seed(3)
        model = create_model("geomx_cnn", image_size=20)
        tr = _trainer(model, sinks)
        for s in range(steps):
            g = torch.Generator().manual_seed(s)
            x = torch.randn(4, 3, 20, 20, generator=g)
            y = torch.randint(0, 10, (4,), generator=g)
            tr.zero_grad()
            F.cross_entropy(model(x), y).backward()
            tr.allreduce_grads()
            for p in model.parameters():
                bk, i = tr.param_bucket[p]
                assert p.grad.data_ptr() == bk.views[i].data_ptr()
            flats = [bk.flat.clone() for bk in tr.buckets]
            tr.update()
        return flats, [p.detach().clone() for p in model.parameters()]

    (fa, pa), (fb, pb) = run(True), run(False)
    for a, b in zip(fa, fb):
        assert torch.equal(a, b)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
