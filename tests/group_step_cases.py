"""Expected values of the grouped optimizer row pushes, shared by test_group_step_cpu.py and
test_gpu_group_step.py.

Nothing here calls the code under test. A grouped optimizer push is the optimizer's replay (adagrad_cases,
rowwise_cases, adam_cases, ftrl_cases) of the contribution rows group_cases.group_contrib builds: the value
row of record i's group as stored or, with coefficients, times coef[i], each product rounded on its own."""
import functools

import numpy as np

from adagrad_cases import replay_adagrad, start_tables
from adam_cases import replay_adam
from ftrl_cases import replay_ftrl
from group_cases import group_coef, group_contrib, group_of, group_records, group_values
from rowwise_cases import replay_rowwise

SIZE = 300
# name -> (PartialMatrix method, BigMatrix method, C symbol of the host form, the scalars in the methods' and
# the replay's order, the scalars in the C order, state parts -- 0: a vector --, replay)
OPT = {
    "adagrad": ("updateRowsAdagrad", "pushAdagrad", "glint_mat_push_rows_adagrad_grouped", (0.05, 1e-6), (0.05, 1e-6),
                1, replay_adagrad),
    "rowwise": ("updateRowsAdagradRowwise", "pushAdagradRowwise", "glint_mat_push_rows_adagrad_rowwise_grouped",
                (0.05, 1e-6), (0.05, 1e-6), 0, replay_rowwise),
    "adam": ("updateRowsAdam", "pushAdam", "glint_mat_push_rows_adam_grouped", (0.05, 1, 0.9, 0.999, 1e-6),
             (0.05, 0.9, 0.999, 1e-6, 1), 2, replay_adam),
    "ftrl": ("updateRowsFtrl", "pushFtrl", "glint_mat_push_rows_ftrl_grouped", (0.1, 1.0, 0.5, 0.01),
             (0.1, 1.0, 0.5, 0.01), 2, replay_ftrl),
}


def start(name, dtype_name, cols, size=SIZE):
    """(w0, s0) of a shard pair: adagrad_cases.start_tables, the state cut to the optimizer's shape; FTRL starts
    from zeros, so that its threshold leaves exact zeros."""
    parts = OPT[name][5]
    if name == "ftrl":
        return np.zeros((size, cols), dtype_name), np.zeros((size, 2 * cols), dtype_name)
    w0 = start_tables(dtype_name, size, cols)[0]
    s0 = start_tables(dtype_name, size, max(parts, 1) * cols)[1]
    return w0, (np.array(s0[:, 0]) if parts == 0 else s0)


def inputs(dtype_name, cols, weighted):
    """The parity push: group_records' 700 records (local rows, offsets), one value row per group and, when
    weighted, one coefficient per record."""
    local, offsets = group_records(SIZE)
    values = group_values(dtype_name, offsets.size - 1, cols)
    return local, offsets, values, group_coef(dtype_name, local.size) if weighted else None


def replay(name, w, s, local, offsets, values, coef=None, order=None):
    """(w', s') after one grouped push: the optimizer's replay of the contribution rows, record by record in
    `order` (default: as given)."""
    contrib = group_contrib(values, group_of(offsets, len(local)), coef)
    if order is not None:
        local, contrib = np.asarray(local)[order], contrib[order]
    return OPT[name][6](w, s, local, contrib, *OPT[name][3])


@functools.lru_cache(maxsize=None)
def case(name, dtype_name, cols, weighted):
    """Both tables after the parity push was applied twice from start(); computed once, read-only."""
    w, s = start(name, dtype_name, cols)
    for _ in range(2):
        w, s = replay(name, w, s, *inputs(dtype_name, cols, weighted))
    w.setflags(write=False)
    s.setflags(write=False)
    return w, s
