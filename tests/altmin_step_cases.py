"""Cases shared by tests/test_altmin_steps_cpu.py and tests/test_altmin_steps.py: instances with their own masks, starts, node sets, and
the references of one V-step and one U-step (oracle/omc_altmin_ref.py).  Not a test module.

A shape is (k, cut type, n, m, fraction observed); its seed is 1000 k + n.  A = L R + 0.01 E as orc.make_instance draws it; the mask is
drawn here so that the edges make_instance redraws away are present:
  column 0 empty, row 0 empty, column 1 observed in every row but row 0, row 1 observed in every column but column 0, column 2 observed
  in row 1 only (n > k + 1; the shapes with n = k, k + 1 keep the empty column, the one-entry column and a full last row: with an empty
  row among k rows the masked matrix has rank k - 1, U0 gets a column that only touches the empty row, V a zero row, and model_U is no
  longer strictly convex).  "Fully observed" is therefore up to the one cell that the empty row or column owns.
The rest is Bernoulli(fraction).  Problems of a shape: start scale s in (0.3, 1, 3) times U0 = svd_rounding, node set c in (no cut, one
cut, two cuts) as in test_altmin_rank_k_matches_oracle; the regular shapes of ranks 1 - 4 take all nine (s, c) (rank 1 needs them for the
coverage conditions of test_altmin_steps_cpu.py), every other shape the diagonal (s_i, c_i) as that test pairs them (a U-step reference
costs about a second at rank 8), and the
shapes with n = k, k + 1 the three scales without cuts: there the symmetry rows already fix the signs of a whole triangle of U, and the
cut bounds around 0.6 U0 on top of them leave model_U without a feasible point (row violation 1.1 - 2.2 in the oracle's U-step)."""
import numpy as np

import omc_altmin_ref as ref
import omc_oracle as orc

GAMMA = 80.0
CUT_TYPES = ["linear", "linear2", "linear3"]
SCALES = [0.3, 1.0, 3.0]

REGULAR = [(k, CUT_TYPES[(k - 1) % 3], 16, 22, 0.6) if k <= 6 else (k, CUT_TYPES[(k - 1) % 3], 20, 26, 0.75) for k in range(1, 9)]
STRIDE = ([(k, CUT_TYPES[k % 3], n, m, 0.2) for k in (1, 2, 4) for (n, m) in ((255, 257), (256, 256), (257, 260))]
          + [(k, CUT_TYPES[k % 3], n, m, 0.2 if n > 64 else 0.5) for k in (5, 8) for (n, m) in ((31, 33), (32, 32), (33, 65), (257, 260))]
          + [(k, CUT_TYPES[k % 3], n, 24, 0.8) for k in (2, 4, 8) for n in (k, k + 1)])
DEGENERATE = [(k, kind) for k in (2, 3, 5) for kind in ("zero_column", "equal_columns")]


def shape_id(s):
    return "k%d-%dx%d" % (s[0], s[2], s[3])


def make_mask(n, m, k, frac, rng):
    mask = rng.random((n, m)) < frac
    mask[:, 2] = False
    if n > k + 1:
        mask[:, 1] = True; mask[1, :] = True
        mask[0, :] = False
    else:
        mask[n - 1, :] = True
    mask[:, 0] = False
    return mask


class Shape:
    """instance, starts and node sets of one shape"""

    def __init__(self, spec, all_pairs):
        self.spec = spec
        self.k, self.cut_type, self.n, self.m, frac = spec
        k, n, m = self.k, self.n, self.m
        rng = np.random.default_rng(1000 * k + n)
        L = rng.standard_normal((n, k)); Rm = rng.standard_normal((k, m)); E = rng.standard_normal((n, m))
        self.A = L @ Rm + 0.01 * E
        self.mask = make_mask(n, m, k, frac, rng)
        self.inst = orc.Instance(self.A, self.mask, GAMMA, k)
        self.U0 = orc.svd_rounding(np.where(self.mask, self.A, 0.0), k)
        dirs = orc.child_directions(self.cut_type, k) if k <= 4 else None
        first = list(dirs[1]) if dirs else _dirs(self.cut_type, k, 1)
        last = list(dirs[-1]) if dirs else _dirs(self.cut_type, k, -1)
        zero = list(dirs[0]) if dirs else _dirs(self.cut_type, k, 0)
        x1 = np.linalg.qr(rng.standard_normal((n, 1)))[0][:, 0]; x2 = np.linalg.qr(rng.standard_normal((n, 1)))[0][:, 0]
        node_sets = [[], [(x1, self.U0 * 0.6, first)], [(x1, self.U0 * 0.6, last), (x2, -self.U0 * 0.3, zero)]]
        pairs = [(s, c) for c in range(3) for s in range(3)] if all_pairs else [(0, 0), (1, 1), (2, 2)] if n > k + 1 else [(0, 0), (1, 0), (2, 0)]
        self.labels = ["s%g-c%d" % (SCALES[s], c) for s, c in pairs]
        self.starts = [SCALES[s] * self.U0 for s, c in pairs]
        self.node_sets = [node_sets[c] for s, c in pairs]
        self._vref = {}; self._uref = {}

    def v_ref(self, p):
        if p not in self._vref:
            self._vref[p] = ref.v_step_ref(self.A, self.mask, GAMMA, self.starts[p])
        return self._vref[p]

    def u_ref(self, p, V=None):
        """U-step reference of problem p for the factor V (default: the V-step reference rounded to float64); kept per (p, V)."""
        V = np.asarray(self.v_ref(p)["V"], np.float64) if V is None else np.asarray(V, np.float64)
        key = (p, V.tobytes())
        if key not in self._uref:
            self._uref[key] = ref.u_step_ref(self.inst, V, self.node_sets[p], self.cut_type)
        return self._uref[key]


def _dirs(cut_type, k, which):
    """child_directions(cut_type, k)[which] for which in (0, 1, -1) without building the labels^k product (3^8, 4^8 lists at k = 8)"""
    labels = orc.DIRECTIONS_OF[cut_type]
    if which == 0:
        return [labels[0]] * k
    if which == -1:
        return [labels[-1]] * k
    return [labels[1]] + [labels[0]] * (k - 1)      # the first column varies fastest


_shapes = {}


def shape(spec):
    if spec not in _shapes:
        _shapes[spec] = Shape(spec, all_pairs=spec in REGULAR and spec[0] <= 4)
    return _shapes[spec]


def degenerate_start(U0, kind):
    U = U0.copy()
    if kind == "zero_column":
        U[:, 1] = 0.0
    else:
        U[:, 1] = U[:, 0]
    return U
