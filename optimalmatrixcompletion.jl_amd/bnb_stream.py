"""Queue-driven counterpart of the reference's branch-and-bound loop (OMC.jl:700-1073) on ONE running solve.

`bnb.branch_and_bound` works in rounds: pop a batch, relax it to its last node, branch.  Here the engine's solve stays open
(omc_relax_hold), the host takes the results of the nodes that have finished (omc_relax_fetch_done), prunes / updates the incumbent /
creates the children exactly as the reference's loop does for one node (OMC.jl:765-1031), and pushes the best open nodes into the
running solve (omc_relax_append) so that the slots never drain while the queue holds work.  Same selection rule (best-first on the
parent's bound), same altmin coin (OMC.jl:856-870), same certified bounds as `bnb.branch_and_bound`; what differs is only WHEN a node
is relaxed relative to its cousins (several hundred nodes are in flight, as with batch > 1 there).  One process (the multi-rank
exchange stays with the round-based driver).  A second handle of the same instance serves altmin, rounding, the objective scans and the
violated-minor scans while the first one is busy with the solve.

With add_Shor_valid_inequalities (rank 1; the keywords, defaults and range checks of `bnb.branch_and_bound`) every node carries
node.Shor_info (OMC.jl:37-40): the open solve is staged with stage_shor behind reserve / reserve_shor, children go in through
append_shor and inherit their parent's list; in iterative mode a split node that wins the coin of OMC.jl:956-967 fetches its X
(fetch_done_shor) and its children carry the list extended by the most violated minors -- a list the running batch does not know
yet, which takes one of the reserved lists.  The list bookkeeping is shor_lists.ShorLists, shared with the round-based driver.  When the
node capacity, the cut depth, the list length or the list capacity of the running solve is used up the driver lets it drain and stages
the next one.
"""
from __future__ import annotations

import heapq
import math
import time

import numpy as np

from .bnb import make_children, child_directions, autotune_rho_scale, compute_gap, left_singular, rank_k_projection
from .shor_lists import ShorLists


def _incumbent_from_U(engine2, A, indices, U, gamma):
    """Best X = U V for a fixed column space (one V-step of OMC.jl:1979-2279, closed form per column):
    v_j = argmin 1/2 sum_{i in Omega_j} (A_ij - U_i v)^2 + 1/(2 gamma) ||U v||^2."""
    n, m = A.shape
    k = U.shape[1]
    G0 = (U.T @ U) / gamma
    V = np.zeros((k, m))
    for j in range(m):
        o = indices[:, j]
        Uo = U[o]
        V[:, j] = np.linalg.solve(Uo.T @ Uo + G0 + 1e-14 * np.eye(k), Uo.T @ A[o, j])
    X = U @ V
    return float(engine2.evaluate_objective(X)), X


def branch_and_bound_streaming(engine, A, indices, *, gap=1e-4, time_limit=3600.0, disjunctive_cuts_type="linear",
                               disjunctive_cuts_breakpoints="smallest_1_eigvec", rho_scale=None, altmin_flag=True,
                               max_altmin_probability=1.0, min_altmin_probability=0.005, altmin_probability_decay_rate=1.1,
                               slots=1024, in_flight_target=None, capacity=1 << 15, depth_reserve=8, seed=0, accel=1,
                               warm_pool_bytes=6 << 30, verbose=False,
                               add_Shor_valid_inequalities=False, Shor_valid_inequalities_noisy_rank1_num_entries_present=(1, 2, 3, 4),
                               add_Shor_valid_inequalities_fraction=1.0, add_Shor_valid_inequalities_iterative=False,
                               max_update_Shor_indices_probability=1.0, min_update_Shor_indices_probability=0.1,
                               update_Shor_indices_probability_decay_rate=1.1, update_Shor_indices_n_minors=100, shor_params=None,
                               shor_warm_start=False, shor_warm_depth=32, shor_list_capacity=1024, objective_cutoff=False,
                               device_branching=False, use_max_steps=False, max_steps=1000000):
    """Queue-driven branch and bound (module docstring).  The Shor keywords are those of bnb.branch_and_bound; shor_list_capacity is the
    number of lists new to a running solve that one epoch reserves room for (iterative mode; the static mode needs none).
    objective_cutoff (off by default): the incumbent is given to the solving handle before every epoch's submit and again whenever it
    improves while the solve runs (Engine.set_cutoff), so that the nodes in flight which the new incumbent prunes end at their next
    certificate check with status 4 (OBJECTIVE_LIMIT); the epoch's clean-up sets the cutoff back to inf.  Such a node is counted in
    nodes_relax_feasible, nodes_relax_feasible_pruned and nodes_relax_cutoff and takes no further part.  The second handle is untouched.
    device_branching (off by default; base mode only, with the Shor keywords it raises): a child whose parent was relaxed in the running solve
    goes in by reference (Engine.append_children: the library builds its descriptor on the device from the parent's) instead of through
    its whole cut list; the host list is still kept, for altmin and for the epoch that restages the node.  The descriptors are the same bit
    for bit, so selection, coins, counters and pruning see the same tree.  counters["nodes_appended_by_reference"] counts those children.
    use_max_steps / max_steps: the node cap of the reference (OMC.jl:128-129, 702) as bnb.branch_and_bound applies it: no new solve is
    staged and nothing more is pushed once nodes_total has reached max_steps.
    instance["relax_log"] lists every relaxed node as (id, status, iterations, how it ended)."""
    from .api import default_params, BREAKPOINTS, Engine
    from .data import compute_MSE
    n, m, k = engine.n, engine.m, engine.k
    shor = bool(add_Shor_valid_inequalities)
    if shor and device_branching:
        raise ValueError("device_branching is for the base mode: a Shor child inherits its parent's list (append_shor)")
    if shor:
        if k > 1:
            raise NotImplementedError("Shor mode of the queue-driven driver is rank 1 (omc_relax_append_shor); rank k > 1 runs in bnb.branch_and_bound")
        lists = ShorLists(Shor_valid_inequalities_noisy_rank1_num_entries_present, add_Shor_valid_inequalities_fraction,
                          add_Shor_valid_inequalities_iterative, max_update_Shor_indices_probability, min_update_Shor_indices_probability,
                          update_Shor_indices_probability_decay_rate, update_Shor_indices_n_minors)
    A = np.asarray(A, float); indices = np.asarray(indices, bool)
    rng = np.random.default_rng(seed)
    start = time.time()
    engine2 = Engine(A, indices, engine.gamma, k, device=getattr(engine, "device", 0))
    engine.tuning_set("OMC_NO_GRAPH", "1")      # two handles work side by side: no stream capture on the solving one while the other issues copies and launches
    counters = dict(nodes_explored=0, nodes_total=1, nodes_dominated=0, nodes_relax_infeasible=0, nodes_relax_feasible=0,
                    nodes_relax_feasible_pruned=0, nodes_master_feasible=0, nodes_master_feasible_improvement=0,
                    nodes_relax_feasible_split=0, nodes_relax_feasible_split_altmin=0, nodes_relax_feasible_split_altmin_improvement=0,
                    warm_started=0, epochs=0)
    if objective_cutoff:
        counters["nodes_relax_cutoff"] = 0
    if device_branching:
        counters["nodes_appended_by_reference"] = 0
    relax_log = []
    epoch_open = False          # a submitted solve runs on `engine`: an improved incumbent goes to it at once
    # ---- root altmin (OMC.jl:521-621) on the second handle ----------------------------------------------------------------
    A0 = np.where(indices, A, 0.0)
    U0 = left_singular(engine2, A0, k)
    solution = {}
    if altmin_flag:
        am = engine2.alternating_minimization([U0], [[]], disjunctive_cuts_type, time_limit=time_limit)[0]      # OMC.jl:545
        X0 = am["U"] @ am["V"]
    else:
        X0 = U0 @ (U0.T @ A0)
    ub = float(engine2.evaluate_objective(X0))
    solution.update(objective_initial=ub, X_initial=X0, objective=ub, X=X0, U=left_singular(engine2, X0, k))
    # ---- penalty scale and root relaxation (the winner of the autotune batch IS the root relaxation) --------------------------
    if shor and rho_scale is None:
        rho_scale = 1.0                      # the Shor splitting has its own (scaled) penalties: no autotune
    if rho_scale is None:
        rho_scale, _, root = autotune_rho_scale(engine, disjunctive_cuts_type, return_result=True, breakpoints=BREAKPOINTS[disjunctive_cuts_breakpoints])
    else:
        root = None
    P = default_params(rho_scale=float(rho_scale), breakpoints=BREAKPOINTS[disjunctive_cuts_breakpoints], accel=int(accel), slots=int(slots))
    root_minors = None
    if shor:
        # as bnb.branch_and_bound: 1e-5 is the tolerance SURVEY 8c states for the Shor configurations
        P = shor_params or default_params(rho_scale=1.0, breakpoints=BREAKPOINTS[disjunctive_cuts_breakpoints], eps_gap=1e-5, max_iters=8000)
        P.slots = int(slots)
        root_minors = lists.root(engine, rng)
        root = engine.matrix_completion_SDP_relaxation([[]], disjunctive_cuts_type, params=P, want_X=True, add_Shor_valid_inequalities=True,
                                                       shor_info=[(root_minors, None)])[0]
    if root is None:
        root = engine.matrix_completion_SDP_relaxation([[]], disjunctive_cuts_type, params=P, want_X=False)[0]
    # ---- warm-start pool: a ring much longer than the in-flight window, entry -> node that owns it -----------------------------
    nnz = int(np.count_nonzero(indices)); np16 = (n + 15) // 16 * 16
    state_bytes = 8 * (3 * n * n + n * k + nnz + m + 16 * np16 + 20)
    target = int(in_flight_target or 2 * slots)
    shor_nq_max = 0
    if shor:
        shor_nq_max = lists.pool_nq_max(root_minors, shor_warm_depth)
        state_bytes += engine.shor_state_bytes(n, m, shor_nq_max)
    pool_cap = int(max(0, min(1 << 16, warm_pool_bytes // state_bytes))) if (not shor or shor_warm_start) else 0
    if pool_cap >= 8 * target:
        engine.state_pool_create(pool_cap)
        if shor:
            engine.state_pool_reserve_shor(shor_nq_max)
    else:
        pool_cap = 0
    pool_next = 0; pool_owner = {}
    altmin_decay_depth = math.log(max_altmin_probability / min_altmin_probability, altmin_probability_decay_rate) if altmin_flag else 0.0

    heap = []          # (LB, id): open nodes, best-first on the parent's certified bound (OMC.jl:1164-1182)
    nodes = {}         # id -> dict(cuts, LB, depth, pstate)
    lb = -math.inf
    t_altmin = 0.0
    t_append = 0.0          # host time inside append / append_shor / append_children (run_details["append_seconds"])
    pending_altmin = []          # (Y, cuts) of split nodes that won the altmin coin: relaxed in batches on the second handle

    def consider(cand_val, cand_X, kind):
        nonlocal ub
        if cand_val < ub:
            ub = cand_val
            solution.update(objective=ub, X=cand_X, U=left_singular(engine2, cand_X, k), objective_time_found=time.time() - start)
            counters["nodes_master_feasible_improvement" if kind == "master" else "nodes_relax_feasible_split_altmin_improvement"] += 1
            for nid in [i for i, nd in nodes.items() if nd["LB"] > ub]:       # prune dominated nodes (OMC.jl:1220-1244)
                del nodes[nid]
            if objective_cutoff and epoch_open:
                engine.set_cutoff(ub)          # the nodes in flight see it at their next certificate check

    def node_X(o):
        """X of a finished Shor node: the root's result carries it, a node of the running solve is fetched (fetch_done_shor)."""
        return o["X"] if "X" in o else engine.fetch_done_shor([o["node"]])[0]["X"]

    def process(nid, nd, o):
        """One node's share of OMC.jl:765-1031."""
        nonlocal lb
        counters["nodes_explored"] += 1
        if o["status_code"] == 3:
            counters["nodes_relax_infeasible"] += 1
            relax_log.append((nid, 3, o["iters"], "infeasible"))
            return
        counters["nodes_relax_feasible"] += 1
        if shor and len(nd["shor"]):
            counters["shor_nodes_with_minors"] = counters.get("shor_nodes_with_minors", 0) + 1
        bound = o["dual_bound"]
        if nid == 1:
            lb = bound
        if o["status_code"] == 4:            # stopped by the cutoff: dual_bound > the incumbent it was given (and ub has not risen since)
            counters["nodes_relax_feasible_pruned"] += 1
            counters["nodes_relax_cutoff"] = counters.get("nodes_relax_cutoff", 0) + 1
            relax_log.append((nid, 4, o["iters"], "cutoff"))
            return
        if bound > ub:
            counters["nodes_relax_feasible_pruned"] += 1
            relax_log.append((nid, o["status_code"], o["iters"], "pruned"))
            return
        if o["status_code"] == 0 and o["lambda_min"][0] >= -1e-6:
            counters["nodes_master_feasible"] += 1
            relax_log.append((nid, 0, o["iters"], "master"))
            if shor:                         # as bnb.branch_and_bound: the master objective of the rank-k projection of the node's X
                Xk, _ = rank_k_projection(node_X(o), k, engine2)
                val = float(engine2.evaluate_objective(Xk))
            else:
                val, Xk = _incumbent_from_U(engine2, A, indices, o["U"], engine.gamma)
            consider(val, Xk, "master")
            return
        counters["nodes_relax_feasible_split"] += 1
        relax_log.append((nid, o["status_code"], o["iters"], "split"))
        if altmin_flag and "Y" in o:
            p = min_altmin_probability if nd["depth"] > altmin_decay_depth else max_altmin_probability / (altmin_probability_decay_rate ** nd["depth"])
            if rng.random() < p:
                counters["nodes_relax_feasible_split_altmin"] += 1
                pending_altmin.append((o["Y"], nd["cuts"]))
        child_shor = None
        if shor:                             # OMC.jl:956-967, 2495-2518; the scan runs on the second handle
            child_shor = lists.child(engine2, nd["shor"], nd["depth"], lambda: node_X(o), rng, k, counters)
        for cuts, dirs in zip(make_children(nd["cuts"], o, disjunctive_cuts_type, k), child_directions(disjunctive_cuts_type, k)):
            counters["nodes_total"] += 1
            cid = counters["nodes_total"]
            nodes[cid] = dict(cuts=cuts, LB=bound, depth=nd["depth"] + 1, pstate=nd.get("state"))
            if device_branching and "node" in o:      # relaxed in a solve of `engine`: (its id there, that solve's epoch, the new cut's directions)
                nodes[cid]["ref"] = (o["node"], counters["epochs"], dirs)
            if shor:
                nodes[cid]["shor"] = child_shor
            heapq.heappush(heap, (bound, cid))

    def run_altmin(force=False):
        nonlocal t_altmin
        if not pending_altmin or (len(pending_altmin) < 8 and not force):
            return
        t0 = time.time()
        batch = pending_altmin[:64]; del pending_altmin[:64]
        Ur = engine2.round_Y([y for y, _ in batch])                                           # OMC.jl:873
        ams = [a for a in engine2.alternating_minimization(Ur, [c for _, c in batch], disjunctive_cuts_type, time_limit=time_limit) if a["converged"]]      # OMC.jl:880, 888
        if ams:
            best = min(ams, key=lambda a: a["master_objective"])
            consider(best["master_objective"], best["U"] @ best["V"], "altmin")
        t_altmin += time.time() - t0

    def pop_best(limit, depth_cap, nq_cap=None, known=None, list_room=0):
        """The best open nodes the running (or next) solve can take: at most `limit`, none deeper than the reserved cut depth; in Shor mode
        none whose list is longer than nq_cap, and at most list_room lists the solve does not know yet (known: id of a list -> the list)."""
        out = []
        while heap and len(out) < limit:
            _, nid = heap[0]
            if nid not in nodes:
                heapq.heappop(heap); continue
            if nodes[nid]["LB"] > ub:
                heapq.heappop(heap); del nodes[nid]; counters["nodes_dominated"] += 1; continue
            if nodes[nid]["depth"] > depth_cap:
                break
            if shor and nq_cap is not None:
                lst = nodes[nid]["shor"]
                if len(lst) > nq_cap:
                    break
                if id(lst) not in known:
                    if list_room <= 0:
                        break
                    list_room -= 1; known[id(lst)] = lst
            heapq.heappop(heap)
            out.append((nid, nodes.pop(nid)))
        return out

    def warm_indices(batch):
        nonlocal pool_next
        if not pool_cap:
            return None, None
        lf = []; sv = []
        fits = [not shor or len(nd["shor"]) <= shor_nq_max for _, nd in batch]      # a Shor list that has outgrown the pool: cold, not saved
        for (nid, nd), fit in zip(batch, fits):
            ps = nd.get("pstate")
            ok = fit and ps is not None and pool_owner.get(ps[0]) == ps[1]
            lf.append(ps[0] if ok else -1)
            if not shor:                     # Shor mode counts the loads the library accepted (shor_warm_stats, at the end of an epoch)
                counters["warm_started"] += 1 if ok else 0
        for (nid, nd), fit in zip(batch, fits):
            if not fit:
                sv.append(-1); counters["shor_warm_outgrown"] = counters.get("shor_warm_outgrown", 0) + 1
                continue
            sv.append(pool_next); pool_owner[pool_next] = nid; nd["state"] = (pool_next, nid); pool_next = (pool_next + 1) % pool_cap
        return lf, sv

    # root: already relaxed; its state is not in the pool (children of the root start cold)
    process(1, dict(cuts=[], LB=-math.inf, depth=0, shor=root_minors), dict(root, Y=root.get("Y")) if root.get("Y") is not None else root)
    run_altmin(force=True)
    now_gap = compute_gap(lb, ub)
    run_log = [(counters["nodes_explored"], counters["nodes_total"], len(nodes), lb, ub, now_gap, time.time() - start)]
    relax_seconds = 0.0

    def open_lb(in_flight):
        while heap and heap[0][1] not in nodes:
            heapq.heappop(heap)
        vals = [heap[0][0]] if heap else []
        vals += [nd["LB"] for _, nd in in_flight.values()]
        return min(vals) if vals else None

    def capped():
        return use_max_steps and counters["nodes_total"] >= max_steps

    while now_gap > gap and not capped() and time.time() - start <= time_limit and nodes:
        # ---- one epoch = one running solve; a new one is staged when the tree outgrows the reserved cut depth or the node capacity ----------
        counters["epochs"] += 1
        best = [nid for _, nid in heapq.nsmallest(slots, heap) if nid in nodes]          # the nodes this epoch starts with decide the cut depth it reserves
        depth_cap = (max(nodes[nid]["depth"] for nid in best) if best else 0) + depth_reserve
        nq_cap = None; known = {}; list_cap = 0
        if shor:
            # the staged lists are free; an epoch of the iterative mode reserves room for lists depth_reserve updates longer than the longest
            # it starts with and for shor_list_capacity lists that the updates of its split nodes will create
            nq_cap = max([len(nodes[nid]["shor"]) for nid in best] + [0]) + (depth_reserve * lists.n_minors if lists.iterative else 0)
            list_cap = int(shor_list_capacity) if lists.iterative else 0
        first = pop_best(slots, depth_cap, nq_cap, known, len(best) + 1)
        if not first:
            break
        n_staged_lists = len(known)
        lf, sv = warm_indices(first)
        P.time_limit = max(1.0, time_limit - (time.time() - start))
        engine.reserve(capacity, depth_cap)
        if shor:
            engine.reserve_shor(nq_cap, list_cap)
            engine.stage_shor([nd["cuts"] for _, nd in first], [(nd["shor"], None) for _, nd in first], disjunctive_cuts_type, P,
                              load_from=lf, save_to=sv)
        else:
            engine.stage([nd["cuts"] for _, nd in first], disjunctive_cuts_type, P, load_from=lf, save_to=sv)
        engine.hold(True)
        t_epoch = time.time()
        if objective_cutoff:
            engine.set_cutoff(ub)
        engine.submit()
        epoch_open = True
        in_flight = {i: first[i] for i in range(len(first))}
        sent = len(first); stop_push = False
        while True:
            got = engine.fetch_done(max_nodes=1024, want_Y=altmin_flag)
            for o in got:
                nid, nd = in_flight.pop(o["node"])
                process(nid, nd, o)
            if got:
                run_altmin()
                v = open_lb(in_flight)
                if v is not None and v > lb:
                    lb = v
                now_gap = compute_gap(lb, ub)
                run_log.append((counters["nodes_explored"], counters["nodes_total"], len(nodes) + len(in_flight), lb, ub, now_gap, time.time() - start))
                if verbose:
                    print("| %10d | %10d | %10d | %10f | %10f | %10f | %10.3f  s  |" % run_log[-1], flush=True)
            done = now_gap <= gap or capped() or time.time() - start > time_limit or (not nodes and not in_flight)
            if done:
                break
            if not stop_push and len(in_flight) < target:
                room = min(target - len(in_flight), capacity - (sent - len(first)))
                snapshot = dict(known) if shor else None
                push = pop_best(room, depth_cap, nq_cap, known, n_staged_lists + list_cap - len(known)) if room > 0 else []
                if push:
                    lf, sv = warm_indices(push)
                    taken = 0
                    t_push = time.time()
                    try:
                        if shor:
                            engine.append_shor([nd["cuts"] for _, nd in push], [(nd["shor"], None) for _, nd in push], disjunctive_cuts_type,
                                               load_from=lf, save_to=sv)
                            taken = len(push)
                        else:
                            # in queue order, so that the ids are the ones one append call would give: runs of children whose parent
                            # belongs to this solve go in by reference, the runs between them through their cut lists
                            by_ref = [device_branching and nd.get("ref") is not None and nd["ref"][1] == counters["epochs"] for _, nd in push]
                            while taken < len(push):
                                end = taken + 1
                                while end < len(push) and by_ref[end] == by_ref[taken]:
                                    end += 1
                                run = push[taken:end]
                                wl = None if lf is None else lf[taken:end]; ws_ = None if sv is None else sv[taken:end]
                                if by_ref[taken]:
                                    engine.append_children([nd["ref"][0] for _, nd in run], [nd["ref"][2] for _, nd in run], load_from=wl, save_to=ws_)
                                    counters["nodes_appended_by_reference"] += len(run)
                                else:
                                    engine.append([nd["cuts"] for _, nd in run], disjunctive_cuts_type, load_from=wl, save_to=ws_)
                                taken = end
                    except Exception:                              # the solve ended on its time limit between our checks: back into the queue
                        if shor:
                            known.clear(); known.update(snapshot)
                        for nid, nd in push[taken:]:
                            nodes[nid] = nd; heapq.heappush(heap, (nd["LB"], nid))
                        stop_push = True
                        push = push[:taken]
                    t_append += time.time() - t_push
                    for q, item in enumerate(push):
                        in_flight[sent + q] = item
                    sent += len(push)
                elif room <= 0 or (heap and nodes):
                    stop_push = True            # capacity used up, or the best open node lies below the reserved depth (Shor: carries a list too long, or a new list when none is left): drain and stage a new solve
            if stop_push and not in_flight:
                break
            if not got:
                time.sleep(0.0005)
        engine.hold(False)
        engine.wait()
        epoch_open = False
        if objective_cutoff:
            engine.set_cutoff(math.inf)          # the handle leaves the epoch as it entered
        for o in engine.fetch_done(max_nodes=1 << 15, want_Y=False):      # nodes that finished after the loop decided to stop: their bounds still count
            if o["node"] in in_flight:
                nid, nd = in_flight.pop(o["node"])
                process(nid, nd, o)
        for nid, nd in in_flight.values():              # (none unless the time limit struck) -- back into the queue
            nodes[nid] = nd; heapq.heappush(heap, (nd["LB"], nid))
        if shor and pool_cap:
            ws = engine.shor_warm_stats()    # accumulated over the staged and the appended nodes of this solve
            counters["warm_started"] += ws["loaded_identical"] + ws["loaded_prefix"]
            counters["shor_warm_refused"] = counters.get("shor_warm_refused", 0) + ws["refused"]
        relax_seconds += time.time() - t_epoch
        run_altmin(force=True)
        v = open_lb({})
        if v is not None and v > lb:
            lb = v
        now_gap = compute_gap(lb, ub)
    elapsed = time.time() - start
    solution.update(lower_bound=lb, gap=now_gap, MSE_in=compute_MSE(solution["X"], A, indices, "in"),
                    MSE_out=compute_MSE(solution["X"], A, indices, "out"), MSE_all=compute_MSE(solution["X"], A, indices, "all"))
    engine2.close()
    engine.tuning_set("OMC_NO_GRAPH", None)
    instance = dict(run_log=run_log, run_log_columns=("explored", "total", "remaining", "lower", "upper", "gap", "runtime"), relax_log=relax_log,
                    run_details=dict(counters, time_taken=elapsed, solve_time_relaxation=relax_seconds, solve_time_altmin=t_altmin, append_seconds=t_append,
                                     rho_scale=float(rho_scale), slots=slots, in_flight_target=target, n=n, m=m, k=k))
    return solution, instance
