"""Case table, input builders and runners of the optimizer goldens (helper,
not a test; used by scripts/record_optim_golden.py,
tests/test_optim_golden_gpu.py and tests/test_optim_golden_cpu.py).

tests/golden/optim_parent.npz holds the result of ONE step of every server
optimizer kernel, dense and row-sparse, recorded on an MI355X from the
commit named in the file's `commit` entry: the last one whose kernels spell
each update rule out by hand. Inputs come from the seeded builders of
tests/kvstore_edge_cases.py (non-zero states), so they are the same bytes
on any machine. The kernels are elementwise: one step fixes the bits.

Keys:
  dense/<variant>/<out>   the outputs of all DENSE_SIZES, concatenated
  big/<variant>/<out>     SHA-256 of the output bytes of the grid-stride
                          wrap case (a one-element string array)
  row/<rule>/<case>/<out> the whole [ROWS][width] table or state
"""

import hashlib
import os

import numpy as np
import torch

import kvstore_edge_cases as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "optim_parent.npz")
SEED = 5
ADAM_T = 2

VARIANTS = sorted(K.OPT_HP)
# 1, 3: tail only; 4, 8, 64: whole vectors only; 5, 7, 63, 65, 255, 257: a
# tail of 1 and of 3 behind one vector, one wave and one block of them;
# 1023: 255 vectors + 3
DENSE_SIZES = (1, 3, 4, 5, 7, 8, 63, 64, 65, 255, 257, 1023)

ROW_RULES = ("sgd", "sgd_mom", "adam", "adagrad")
ROWS, SLOTS = 24, 20
ROW_SKIPPED = (-1, -1, -1, 24, 29, -7)     # padding and out-of-range ids
# (width, offset view): 5 scalar path; 8 vector path; 64 vector path on
# more than one block; 8 as views one element into a larger buffer, which
# are not 16-byte aligned and take the scalar path
ROW_CASES = ((5, False), (8, False), (64, False), (8, True))


def outputs(name):
    return ["w"] + K.OPT_STATES[name]


def hp_of(name):
    return dict(K.OPT_HP[name], t=ADAM_T)


def big_n(name):
    return K.OPT_BIG_FLOAT4 if name in K.OPT_FLOAT4 else K.OPT_BIG_SCALAR


def dense_case(name, n):
    """(state0 dict of fp32 arrays, g)."""
    st, gs = K.opt_case(name, n, seed=SEED, steps=1)
    return st, gs[0]


def row_tag(width, offset):
    return "w%d%s" % (width, "_offset" if offset else "")


def row_case(rule, width):
    """(state0 dict of [ROWS][width] fp32 arrays, ids int64 [SLOTS], merged
    [SLOTS][width]): unique in-range ids and ROW_SKIPPED, shuffled."""
    st, gs = K.opt_case(rule, ROWS * width, seed=SEED + 1, steps=1)
    st = {k: v.reshape(ROWS, width) for k, v in st.items()}
    merged = gs[0].reshape(ROWS, width)[:SLOTS].copy()
    rng = np.random.default_rng(1000 * width + len(rule))
    live = rng.permutation(ROWS)[:SLOTS - len(ROW_SKIPPED)]
    ids = rng.permutation(np.concatenate([live, ROW_SKIPPED]))
    return st, ids.astype(np.int64), merged


def row_valid(ids):
    return (ids >= 0) & (ids < ROWS)


def row_call(mod, rule, st, ids, merged, hp):
    """One row-indexed step through `mod` (geomx_amd.ops or its reference
    module), in place on the torch tensors of `st`."""
    lr, wd, rs = hp["lr"], hp["wd"], hp["rescale"]
    w = st["w"]
    if rule == "sgd":
        mod.rsp_sgd_update(w, ids, merged, lr, wd, rs)
    elif rule == "sgd_mom":
        mod.rsp_sgd_mom_update(w, ids, merged, st["mom"], lr,
                               hp["momentum"], wd, rs)
    elif rule == "adam":
        mod.rsp_adam_update(w, ids, merged, st["m"], st["v"], hp["t"], lr,
                            hp["beta1"], hp["beta2"], hp["eps"], wd, rs)
    else:
        mod.rsp_adagrad_update(w, ids, merged, st["h"], lr, hp["eps"], wd,
                               rs)


def _offset_view(t):
    # from the test module, not kvstore_edge_cases: the goldens are checked
    # by re-recording on the parent commit with only this module and the
    # record script added, and the parent has the helper only there
    from test_kvstore_kernels_edges_gpu import _offset_view as view
    return view(t)


def run_dense(mod, name, st0, g, device="cpu"):
    """One dense step from copies of st0; {out: fp32 array}."""
    st = {k: torch.from_numpy(v.copy()).to(device) for k, v in st0.items()}
    K.opt_call(mod, name, st, torch.from_numpy(g).to(device), hp_of(name))
    return {k: v.cpu().numpy() for k, v in st.items()}


def row_operands(st0, ids, merged, offset, device="cpu"):
    """Torch operands of a row case on `device`; with `offset`, table,
    states and merged rows are views one element into a larger buffer."""
    place = _offset_view if offset else (lambda t: t)
    st = {k: place(torch.from_numpy(v.copy()).to(device))
          for k, v in st0.items()}
    return (st, torch.from_numpy(ids).to(device),
            place(torch.from_numpy(merged.copy()).to(device)))


def run_row(mod, rule, st0, ids, merged, offset, device="cpu"):
    """One row-indexed step from copies of st0; {out: [ROWS][width]}."""
    st, ids_t, merged_t = row_operands(st0, ids, merged, offset, device)
    row_call(mod, rule, st, ids_t, merged_t, hp_of(rule))
    return {k: v.cpu().numpy() for k, v in st.items()}


def digest(a):
    return hashlib.sha256(
        np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def split_dense(flat):
    """The concatenated golden of one output -> {n: array}."""
    ends = np.cumsum(DENSE_SIZES)
    assert flat.size == ends[-1]
    return {n: flat[e - n:e] for n, e in zip(DENSE_SIZES, ends)}
