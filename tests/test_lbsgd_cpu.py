"""LBSGD on the CPU route: the golden model against a float64 transcription
of the reference formulas (_get_lars, _get_lbmult), the spec round trip, and
a GeoTrainer step whose LARS layers are the parameters."""

import math
import pickle

import pytest
import torch

from geomx_amd import Config, ops
from geomx_amd.kvstore.optimizer import OptimizerSpec, ServerOptimizer
from geomx_amd.ops import reference as ref
from geomx_amd.parallel import GeoTrainer
from geomx_amd.topology import init_topology

STRATEGIES = ("linear", "power2", "sqrt", "lars")


def _get_lars(w, g, wd):
    w2 = math.fsum(float(x) * float(x) for x in w)
    g2 = math.fsum(float(x) * float(x) for x in g)
    return min(max(math.sqrt(w2 / (g2 + wd * w2 + 1e-18)), 0.01), 100.0)


def _get_lbmult(strategy, nup, warmup_epochs, updates_per_epoch, batch_scale):
    nwup = warmup_epochs * updates_per_epoch
    if nup >= nwup:
        return float(batch_scale)
    if nwup <= 1:
        return 1.0
    frac = {"linear": nup / nwup, "power2": nup * nup / (nwup * nwup),
            "sqrt": math.sqrt(nup / nwup), "lars": 0.0}[strategy]
    return 1.0 + (batch_scale - 1) * frac


def test_lars_ratio_is_the_reference_formula():
    torch.manual_seed(0)
    seg = torch.tensor([0, 5, 5, 300, 310, 330, 400])
    w, g = torch.randn(400), torch.randn(400)
    w[300:310] = 0.0            # |w| = 0: clamped to 0.01
    g[310:330] *= 1e-6          # |g| tiny against |w|: clamped to 100
    for wd in (0.0, 0.1):
        want = [_get_lars(w[a:b], g[a:b], wd)
                for a, b in zip(seg[:-1].tolist(), seg[1:].tolist())]
        got = ref.lars_ratio(w, g, seg, wd, dtype=torch.float64)
        assert got.tolist() == pytest.approx(want, rel=1e-14)
        assert got[1] == 0.01 and got[3] == 0.01
        assert got[4] == 100.0 or wd > 0   # wd caps the ratio at wd^-1/2
        assert torch.equal(ops.lars_ratio(w, g, seg, wd), got.float())


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("momentum", (0.0, 0.9))
def test_server_optimizer_follows_the_schedule(strategy, momentum):
    torch.manual_seed(1)
    spec = OptimizerSpec("lbsgd", lr=0.1, momentum=momentum, wd=0.01,
                         warmup_strategy=strategy, warmup_epochs=2,
                         updates_per_epoch=3, batch_scale=4, begin_epoch=1)
    opt = ServerOptimizer(spec)
    w = torch.randn(50)
    w_ref, mom = w.double(), torch.zeros(50, dtype=torch.float64)
    for t in range(1, 6):    # crosses the end of the warm-up at nup = 6
        g = torch.randn(50)
        opt.update("k", w, g, rescale=0.5)
        mult = _get_lbmult(strategy, t + 3, 2, 3, 4)
        assert ref.lbsgd_lbmult(t + 3, strategy, 2, 3, 4) == \
            pytest.approx(mult, rel=1e-15)
        if strategy == "lars":
            mult = _get_lars(w_ref, g, 0.01)
        step = 0.1 * mult * (g.double() * 0.5 + 0.01 * w_ref)
        mom = momentum * mom - step
        w_ref = w_ref + mom
        torch.testing.assert_close(w, w_ref.float(), rtol=1e-5, atol=1e-6)
    assert ("mom" in opt.state["k"]) == (momentum != 0.0)


def test_spec_round_trip_and_old_blobs():
    spec = OptimizerSpec("lbsgd", warmup_strategy="lars", batch_scale=8)
    opt = ServerOptimizer(spec)
    opt.update("k", torch.ones(4), torch.ones(4))
    blob = pickle.loads(pickle.dumps(opt.state_dict()))
    back = ServerOptimizer(OptimizerSpec("sgd"))
    back.load_state_dict(blob)
    assert back.spec == spec and back.step_count == {"k": 1}
    assert pickle.loads(pickle.dumps(spec)) == spec
    # a blob from before the lbsgd fields existed
    old = ServerOptimizer(OptimizerSpec("sgd_mom", lr=0.3)).state_dict()
    for name in ("warmup_strategy", "warmup_epochs", "batch_scale",
                 "updates_per_epoch", "begin_epoch"):
        del old["spec"][name]
    back.load_state_dict(old)
    assert back.spec == OptimizerSpec("sgd_mom", lr=0.3)
    with pytest.raises(ValueError):
        OptimizerSpec("lbsgd", warmup_strategy="cosine").validate()
    with pytest.raises(ValueError):
        OptimizerSpec("lbsgd", batch_scale=0).validate()


def test_trainer_layers_are_the_parameters():
    torch.manual_seed(2)
    model = torch.nn.Sequential(torch.nn.Linear(7, 9), torch.nn.Tanh(),
                                torch.nn.Linear(9, 3))
    before = [p.detach().clone() for p in model.parameters()]
    cfg = Config.from_env(backend="gloo", device="cpu", bucket_mb=1)
    topo = init_topology(1, None, None, "cpu")
    trainer = GeoTrainer(model, cfg, topo, OptimizerSpec(
        "lbsgd", lr=0.1, momentum=0.9, wd=0.01, warmup_strategy="lars"))
    assert trainer.buckets[0].seg_off.tolist() == [0, 64, 128, 192, 256]
    x, y = torch.randn(8, 7), torch.randint(0, 3, (8,))
    moms = [torch.zeros_like(p) for p in before]
    for _ in range(2):
        trainer.zero_grad()
        torch.nn.functional.cross_entropy(model(x), y).backward()
        grads = [p.grad.detach().clone() for p in model.parameters()]
        trainer.step()
        for p, w, g, m in zip(model.parameters(), before, grads, moms):
            ref.lbsgd_update(w, g, m, torch.tensor([0, w.numel()]), 0.1, 0.9,
                             0.01)
            assert torch.equal(p.detach(), w)
    flat = trainer.buckets[0].param_flat   # the padding stayed zero
    assert not flat[3:64].any() and not flat[64 + 27:128].any()
