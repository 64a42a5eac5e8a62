"""Bi-Sparse boundary select (csrc/bscselect.hip) on gfx950: the k-th largest
sampled magnitude from k_bsc_boundary against a CPU sort, bit for bit. Every
step of the key is one IEEE operation or a selection, so there is no
tolerance. Fails without the kernel: neither _geops.bsc_boundary nor
ops.bsc_boundary exists."""
import pytest
import torch

import kvstore_edge_cases as K
from geomx_amd import ops
from geomx_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, MU = 5000, K.BSC_MU
CAP = ops.BSC_BOUNDARY_CAP or 32768  # form one's capacity; None unbuilt
CAND = 8192                          # candidate keys form many holds in LDS
SIZES = (1, 5, 63, 64, 65, 1000, 4097, CAND + 8, CAP + 1)
PAIR = (torch.arange(N) % 3 == 0).float() + 1.0   # 2.0 on a third, else 1.0
SPECIAL = torch.tensor([0.0, -0.0, 1e-45, -3e-39, 1e-38, float("inf"),
                        -float("inf"), 1.5, -2.5, 3e38]).repeat(N // 10)
DATA = {   # name -> v of N elements from a seeded generator
    "normal": lambda g: torch.randn(N, generator=g),
    "equal": lambda g: torch.full((N,), -0.75),
    "two_values": lambda g: PAIR.clone(),         # k lands in either group
    "one_bin": lambda g: 1 + torch.rand(N, generator=g) * 2.0 ** -5,
    "wide": lambda g: torch.randn(N, generator=g)
    * 10.0 ** (60 * torch.rand(N, generator=g) - 30),
    "special": lambda g: SPECIAL.clone(),
}


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("n_wg", (1, 2, 7, 0))
def test_kernel_equals_cpu_sort(n_wg, S):
    if n_wg == 1 and S > CAP:
        pytest.skip("over the one-workgroup form's capacity")
    gen = torch.Generator().manual_seed(S)
    si = torch.randint(0, N, (S,), generator=gen)   # with replacement
    g = 0.5 * torch.randn(N, generator=gen)
    u = 0.5 * torch.randn(N, generator=gen)
    si_d, g_d, u_d = si.int().to(DEV), g.to(DEV), u.to(DEV)
    out = torch.empty(1, device=DEV)
    for name, make in DATA.items():
        v = make(gen)
        v_d = v.to(DEV)
        for mom in (True, False):
            c = (v[si] + (u[si] * MU + g[si])).abs() if mom else v[si].abs()
            want = torch.sort(c, descending=True).values
            gu = (g_d, u_d) if mom else (torch.Tensor(), torch.Tensor())
            for k in sorted({1, min(2, S), max(1, S // 100),
                             max(1, S // 2), S}):
                ops._geops.bsc_boundary(v_d, *gu, si_d, k, MU, out, n_wg)
                got = out.cpu()
                assert torch.equal(got.view(torch.int32),
                                   want[k - 1:k].view(torch.int32)), \
                    (name, mom, k, got.item(), want[k - 1].item())


@pytest.mark.parametrize("n_wg", (1, 5, 0))
def test_flip_element_is_the_boundary(n_wg):
    """The k-th sample is the element whose fused multiply-add differs from
    multiply-then-add: the key is rounded in two steps."""
    c = K.bsc_flip_case()
    n = c["v"].numel()
    S = min(ref.bsc_sample_size(n, K.FLIP_RATIO), n)
    si = ref.bsc_sample_indices(n, S, 42).int().to(DEV)
    out = torch.empty(1, device=DEV)
    ops._geops.bsc_boundary(c["v"].to(DEV), c["g"].to(DEV), c["u"].to(DEV),
                            si, int(S * K.FLIP_RATIO), MU, out, n_wg)
    assert out.item() == c["sep"] != c["fma"]


def test_back_to_back_calls_are_independent():
    """Three ticket-form calls on one stream with no synchronize between
    them: each has its own zeroed histogram and ticket."""
    gen = torch.Generator().manual_seed(9)
    vs = [torch.randn(N, generator=gen) * s for s in (1.0, 100.0, 0.01)]
    si = torch.randint(0, N, (4097,), generator=gen)
    si_d = si.int().to(DEV)
    vs_d = [v.to(DEV) for v in vs]
    outs = [torch.empty(1, device=DEV) for _ in vs]
    for v_d, out in zip(vs_d, outs):
        ops._geops.bsc_boundary(v_d, torch.Tensor(), torch.Tensor(), si_d, 40,
                                MU, out, 7)
    for v, out in zip(vs, outs):
        want = torch.sort(v[si].abs(), descending=True).values[39:40]
        assert torch.equal(out.cpu(), want)


# (5 * 2^20, 0.01): S = 26214, over the launcher's switch to the ticket form
@pytest.mark.parametrize("n,ratio", [(37, 0.5), (5, 0.01), (1000, 1.0),
                                     (40000, 0.01), (5 << 20, 0.01)])
def test_op_equals_reference(n, ratio):
    gen = torch.Generator().manual_seed(n)
    v, g, u = (torch.randn(n, generator=gen) for _ in range(3))
    got = ops.bsc_boundary(v.to(DEV), ratio)
    assert got.shape == (1,) and got.dtype == torch.float32 and got.is_cuda
    assert got.data_ptr() % 16 == 0
    assert torch.equal(got.cpu(), torch.tensor([ref.bsc_boundary(v, ratio)]))
    assert torch.equal(ops.bsc_boundary(v, ratio), got.cpu())   # CPU route
    got = ops.bsc_boundary(v.to(DEV), ratio, g=g.to(DEV), u=u.to(DEV))
    post = v + (u * ref.BSC_MOMENTUM + g)
    assert torch.equal(got.cpu(), torch.tensor([ref.bsc_boundary(post, ratio)]))
    strided = torch.randn(n, 2, generator=gen)[:, 0]   # not served: ATen route
    assert torch.equal(ops.bsc_boundary(strided.to(DEV), ratio).cpu(),
                       torch.tensor([ref.bsc_boundary(strided, ratio)]))


def test_bad_operands_raise():
    v = torch.randn(N, device=DEV)
    si = torch.arange(100, dtype=torch.int32, device=DEV)
    out = torch.empty(1, device=DEV)
    none = torch.Tensor()
    for bad in (
            dict(k=0), dict(k=101), dict(si=si.long()), dict(v=v.cpu()),
            dict(v=torch.randn(N, 2, device=DEV)[:, 0]),
            dict(si=torch.arange(CAP + 1, dtype=torch.int32, device=DEV),
                 n_wg=1)):
        a = {**dict(v=v, si=si, k=10, n_wg=0), **bad}
        with pytest.raises(RuntimeError):
            ops._geops.bsc_boundary(a["v"], none, none, a["si"], a["k"], MU,
                                    out, a["n_wg"])
