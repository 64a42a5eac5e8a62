"""The fused classifier tail (ops/fc.py: _MlpTailFn) and its multi-tensor
cast kernels (csrc/finalize.hip).

The tail runs the library GEMMs and reductions eager autograd runs, on
the same operands, and its own kernels only convert values, so every
comparison is torch.equal on integer views: against the eager
Sequential under bf16 autocast, and against the per-tensor casts.
Gradient destinations sit inside sentinel-filled buffers with guards.
"""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import geomx_amd.ops as ops
from geomx_amd import gradsink
from geomx_amd.ops.fc import mlp_tail, tail_route

DEV = "cuda:0"
SENT = 0x7B7B7B7B
GUARD = 96


@pytest.fixture
def geops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.native_available(), \
        f"native extension missing on GPU box: {ops.native_error()}"
    from geomx_amd import _geops
    return _geops


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2
                               else torch.int32)


def _layers(seed):
    torch.manual_seed(seed)
    return nn.Linear(256, 128).to(DEV), nn.Linear(128, 10).to(DEV)


def _input(N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 256, generator=g).to(DEV, torch.bfloat16)
    dy = torch.randn(N, 10, generator=g).to(DEV, torch.bfloat16)
    return x, dy


def _eager(N):
    fc2, fc3 = _layers(3)
    x, dy = _input(N, 40 + N)
    x.requires_grad_(True)
    seq = nn.Sequential(nn.ReLU(), fc2, nn.ReLU(), fc3)
    with torch.autocast("cuda", torch.bfloat16):
        y = seq(x)
    y.backward(dy)
    return y.detach(), x.grad, [p.grad for p in (fc2.weight, fc2.bias,
                                                 fc3.weight, fc3.bias)]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3, 512])
def test_tail_matches_eager(geops, N):
    y_ref, gx_ref, gp_ref = _eager(N)
    fc2, fc3 = _layers(3)
    params = (fc2.weight, fc2.bias, fc3.weight, fc3.bias)
    x, dy = _input(N, 40 + N)
    x.requires_grad_(True)

    # run 1: no sinks, the gradients arrive in fresh tensors
    with torch.autocast("cuda", torch.bfloat16):
        assert tail_route(x, fc2, fc3)
        y = mlp_tail(x, fc2, fc3)
    assert y.dtype == torch.bfloat16
    y.backward(dy)
    assert torch.equal(_bits(y), _bits(y_ref))
    assert torch.equal(_bits(x.grad), _bits(gx_ref))
    for p, g in zip(params, gp_ref):
        assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape
        assert torch.equal(_bits(p.grad), _bits(g))

    # run 2: every parameter has an armed sink over a sentinel buffer,
    # at element offsets 0, 1, 64 and 3 behind the guard
    x.grad = None
    bufs = []
    for p, lead in zip(params, (0, 1, 64, 3)):
        p.grad = None
        n = p.numel()
        buf = torch.full((GUARD + lead + n + GUARD,), SENT,
                         dtype=torch.int32, device=DEV)
        flat = buf.view(torch.float32)
        off = GUARD + lead
        sink = gradsink.GradSink(flat, flat[off:off + n].view(p.shape), p)
        gradsink.attach(p, sink)
        sink.arm()
        bufs.append((buf, off, n, sink))
    with torch.autocast("cuda", torch.bfloat16):
        y = mlp_tail(x, fc2, fc3)
    y.backward(dy)
    assert torch.equal(_bits(y), _bits(y_ref))
    assert torch.equal(_bits(x.grad), _bits(gx_ref))
    for p, g, (buf, off, n, sink) in zip(params, gp_ref, bufs):
        assert p.grad.data_ptr() == sink.data_ptr()   # adopted, not copied
        assert not sink.armed
        want = torch.zeros_like(g)
        want += g                                     # the parent's 0 + x
        assert torch.equal(buf[off:off + n], want.view(-1).view(torch.int32))
        assert bool((buf[:off] == SENT).all())
        assert bool((buf[off + n:] == SENT).all())
        gradsink.detach(p)


@pytest.mark.gpu
def test_cast_many_kernels(geops):
    g = torch.Generator().manual_seed(5)
    sizes = [(128, 256), (128,), (10, 128), (10,), (1,), (257, 3), (1031,),
             (2, 2)]
    src = [torch.randn(*s, generator=g) for s in sizes]
    # ties, denormals, +-0, +-inf and the largest finite among the values
    plants = torch.tensor([0, -(1 << 31), 0x7F800000, -0x00800000,
                           0x00000001, 0x3F808000, 0x3F818000, 0x3F808001,
                           0x3F807FFF, 0x7F7FFFFF], dtype=torch.int32)
    src[0].view(-1).view(torch.int32)[:plants.numel()] = plants
    src[6].view(torch.int32)[-plants.numel():] = plants
    src = [s.to(DEV) for s in src]
    got = geops.cast_many_f32_bf16(src)
    assert len(got) == len(src)
    for s, b in zip(src, got):
        assert b.dtype == torch.bfloat16 and b.shape == s.shape
        assert torch.equal(_bits(b), _bits(s.to(torch.bfloat16)))
    # back, into sentinel-guarded destinations; -0 comes out as +0
    dsts, bufs = [], []
    for k, b in enumerate(got):
        n, lead = b.numel(), (0, 1, 64, 3, 5, 2, 7, 1)[k]
        buf = torch.full((GUARD + lead + n + GUARD,), SENT,
                         dtype=torch.int32, device=DEV)
        off = GUARD + lead
        dsts.append(buf.view(torch.float32)[off:off + n].view(b.shape))
        bufs.append((buf, off, n))
    assert geops.cast_many_bf16_f32_into(got, dsts) is None
    for b, d, (buf, off, n) in zip(got, dsts, bufs):
        want = torch.zeros(b.shape, device=DEV)
        want += b.float()
        assert torch.equal(_bits(d), _bits(want))
        assert bool((buf[:off] == SENT).all())
        assert bool((buf[off + n:] == SENT).all())
    assert not bool((_bits(dsts[0]) == -(1 << 31)).any())
    # clearing: the ranges and nothing else
    geops.zero_many_f32(dsts)
    for d, (buf, off, n) in zip(dsts, bufs):
        assert not bool(buf[off:off + n].any())
        assert bool((buf[:off] == SENT).all())
        assert bool((buf[off + n:] == SENT).all())
    with pytest.raises(RuntimeError):   # 9 tensors
        geops.cast_many_f32_bf16(src + src[:1])
    with pytest.raises(RuntimeError):   # lengths differ
        geops.cast_many_bf16_f32_into(got[:1], dsts[1:2])


# ---------------------------------------------------------------------
# the tail alone under a trainer
# ---------------------------------------------------------------------

class _Tail(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc2 = nn.Linear(256, 128)
        self.fc3 = nn.Linear(128, 10)

    def grad_sink_parameters(self):
        return (self.fc2.weight, self.fc2.bias, self.fc3.weight,
                self.fc3.bias)

    def forward(self, x):
        return mlp_tail(x, self.fc2, self.fc3)


def _train(sinks, steps):
    from geomx_amd import Config
    from geomx_amd.kvstore.optimizer import OptimizerSpec
    from geomx_amd.parallel import GeoTrainer
    from geomx_amd.topology import init_topology
    torch.manual_seed(11)
    model = _Tail().to(DEV)
    tr = GeoTrainer(model, Config.from_env(),
                    init_topology(1, None, None, DEV),
                    OptimizerSpec("sgd_mom", lr=0.05, momentum=0.9),
                    grad_sinks=sinks)
    assert len(tr.sinks) == (4 if sinks else 0)
    flats = []
    for s in range(steps):
        g = torch.Generator().manual_seed(200 + s)
        x = torch.randn(5, 256, generator=g).to(DEV, torch.bfloat16)
        y = torch.randint(0, 10, (5,), generator=g).to(DEV)
        with torch.autocast("cuda", torch.bfloat16):
            loss = F.cross_entropy(model(x), y)
        tr.zero_grad()
        loss.backward()
        for p in model.parameters():
            b, i = tr.param_bucket[p]
            assert p.grad.data_ptr() == b.views[i].data_ptr()
        flats.append([b.flat.clone() for b in tr.buckets])
        tr.step()
    return flats, [p.detach().clone() for p in model.parameters()], tr


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 3])
def test_trainer_tail_sinks_bit_equal(geops, steps):
    fa, pa, tr = _train(True, steps)
    fb, pb, _ = _train(False, steps)
    assert all(not b.clear and not b.gaps for b in tr.buckets)
    for sa, sb in zip(fa, fb):
        for a, b in zip(sa, sb):
            assert torch.equal(_bits(a), _bits(b))
    for a, b in zip(pa, pb):
        assert torch.equal(_bits(a), _bits(b))
