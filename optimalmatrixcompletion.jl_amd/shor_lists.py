"""Bookkeeping of node.Shor_info.constraints_indexes in the two driver counterparts (bnb.branch_and_bound, bnb_stream.
branch_and_bound_streaming): which minors the root carries, when a split node updates the list its children inherit, and how long a
list the warm-start pool is sized for.  One place, so that the two drivers, fed the same random stream, build the same lists.

Static mode (OMC.jl:646-669): the class lists of generate_rank1_matrix_completion_Shor_constraints_indexes (on the device), thinned by the
fraction with numpy's RNG (randsubseq, OMC.jl:652-655).  Iterative mode (OMC.jl:670-674, 956-967, 2495-2518): the root starts without
minors and a split node adds, with probability p(depth), the n_minors most violated minors of its X (generate_violated_Shor_minors on
the device) BEHIND the list it carries -- a child's list has its parent's as a prefix.  The SOC list is always "every coordinate
outside the minors" (OMC.jl:656-665, 2508-2517), which the engine takes as the shorthand None."""
from __future__ import annotations

import math

import numpy as np


class ShorLists:
    def __init__(self, classes=(1, 2, 3, 4), fraction=1.0, iterative=False, max_update_probability=1.0, min_update_probability=0.1,
                 update_probability_decay_rate=1.1, n_minors=100):
        """The Shor keywords of the reference driver with its range checks (OMC.jl:256-263, 297-324)."""
        if not 0.0 <= fraction <= 1.0:
            raise ValueError("Argument `add_Shor_valid_inequalities_fraction` out of bounds [0.0, 1.0].")          # OMC.jl:256-263
        if iterative:
            if not 0.0 <= max_update_probability <= 1.0:
                raise ValueError("Argument `max_update_Shor_indices_probability` out of bounds [0.0, 1.0].")       # OMC.jl:297-303
            if not 0.0 < min_update_probability < 1.0:
                raise ValueError("Argument `min_update_Shor_indices_probability` out of bounds (0.0, 1.0).")       # OMC.jl:304-310
            if not 1.0 < update_probability_decay_rate:
                raise ValueError("Argument `update_Shor_indices_probability_decay_rate` out of bounds (1.0, inf).")   # OMC.jl:311-317
            if not 1 <= n_minors:
                raise ValueError("Argument `update_Shor_indices_n_minors` out of bounds [1.0, inf).")              # OMC.jl:318-324
        self.classes = [int(c) for c in classes]
        self.fraction = float(fraction); self.iterative = bool(iterative)
        self.max_p = max_update_probability; self.min_p = min_update_probability; self.decay = update_probability_decay_rate
        self.n_minors = int(n_minors)
        self.decay_depth = math.log(self.max_p / self.min_p, self.decay) if self.iterative else 0.0

    def root(self, engine, rng):
        """The root's list, an int64 array (count, 4) of 1-based (i1, i2, j1, j2)."""
        if self.iterative:
            return np.zeros((0, 4), np.int64)                                                  # OMC.jl:670-674
        minors = np.asarray(engine.generate_rank1_matrix_completion_Shor_constraints_indexes(self.classes), np.int64).reshape(-1, 4)
        if self.fraction < 1.0:                                                                # randsubseq, OMC.jl:652-655
            minors = minors[rng.random(len(minors)) < self.fraction]
        return minors

    def update_probability(self, depth):
        """p(depth) of OMC.jl:956-967."""
        return self.min_p if depth > self.decay_depth else self.max_p / (self.decay ** depth)

    def child(self, engine, parent_list, depth, get_X, rng, k=1, counters=None):
        """The list the children of a split node at `depth` inherit.  Static mode: the parent's, no coin.  Iterative mode: one coin of
        `rng`; when it wins, get_X() -- the node's relaxed X (n, m), asked for only then -- is scanned on `engine` and the new minors go
        behind the parent's (the union of OMC.jl:2504-2507: the scan excludes the existing ones).  Returns the parent's array itself when
        nothing was added, so that `is` tells an inherited list from a new one."""
        if not self.iterative:
            return parent_list
        if not rng.random() < self.update_probability(depth):
            return parent_list
        X = np.asarray(get_X(), float)
        n, m = X.shape
        # OMC.jl:2497 passes reshape(X, (1, n, m)) whatever k is: the score is the minor of X itself (also what the k > 1 extension
        # Xt_1 = X, Xt_t = 0 gives); the device routine takes (k, n, m)
        X3 = np.zeros((k, n, m)); X3[0] = X
        new = engine.generate_violated_Shor_minors(X3, self.classes, [tuple(t) for t in parent_list.tolist()], self.n_minors)
        add = np.asarray([t for _, t in new], np.int64).reshape(-1, 4)
        if counters is not None:
            counters["shor_updates"] = counters.get("shor_updates", 0) + 1
        return np.concatenate([parent_list, add]) if len(add) else parent_list

    def pool_nq_max(self, root_list, warm_depth):
        """Minors a warm-start pool entry is sized for: the root's list plus warm_depth updates."""
        return len(root_list) + (int(warm_depth) * self.n_minors if self.iterative else 0)
