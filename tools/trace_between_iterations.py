"""What happens between the ADMM iterations, from the compact trace copy that trace_timeline.py writes (start,end,kernel,queue,workgroups
per line, gzip), between the two marker launches: per check the time from the end of its last kernel to the first kernel of the next
iteration; per harvest the time from the end of the check to the end of k_setup (or of k_harvest when no slot is refilled), split into the
gap before the first harvest kernel, the harvest kernels, the gap between k_harvest and k_setup, and k_setup; per harvest, synchronous or
asynchronous, the time from its first kernel's start to the first kernel of the next iteration (an asynchronous harvest's k_harvest ends
after the next k_global has started: its kernels run beside the interval, and the line is near zero or negative); and the durations of
the kernels of that path.
usage: trace_between_iterations.py <trace.csv.gz> [marker kernel] [out.txt]"""
import gzip
import sys

import numpy as np

path = sys.argv[1]
marker = sys.argv[2] if len(sys.argv) > 2 else "k_eval_objective"
rows = []
with gzip.open(path, "rt") as fh:
    for ln in fh:
        f = ln.rstrip("\n").split(",")                  # a template kernel's name holds commas of its own
        rows.append((int(f[0]), int(f[1]), ",".join(f[2:-2]).strip()))
rows.sort()
mk = [i for i, r in enumerate(rows) if marker in r[2]]
if len(mk) >= 2:
    rows = rows[mk[0] + 1:mk[-1]]
K = [r for r in rows if r[2].startswith("k_")]          # kernels of the library (copies and fills left out)
CHECK = ("k_zero_check", "k_colprox", "k_check_build", "k_cone_ws", "k_cone<", "k_cone_sub<1>", "k_check_final", "k_rho_rescale", "k_aa", "k_shor")
HARV = ("k_state_save", "k_small", "k_sep_prepare", "k_cone_sub<2>", "k_cone<true>", "k_harvest", "k_shor")
us = lambda a: np.asarray(a, float) / 1e3
HARV_ONLY = ("k_state_save", "k_sep_prepare", "k_cone_sub<2>", "k_cone<true>", "k_harvest")      # k_small also runs in every iteration
ITER = ("k_cone_sub<0>", "k_colprox_pair", "k_global")
bubble, h_gap1, h_kern, h_gap2, h_setup, h_total, h_next, h_gram = [], [], [], [], [], [], [], []
hs_sync, hs_async, a_kern = [], [], []
i = 0
while i < len(K):
    if not K[i][2].startswith("k_zero_check"):
        i += 1
        continue
    j = i                                               # the check's kernels: up to its last k_check_final / k_rho_rescale / k_aa
    last = None
    while j < len(K) and (K[j][2].startswith(CHECK) or K[j][2].startswith("k_setup_gram")) and not K[j][2].startswith(("k_cone_sub<2>", "k_cone<true>")):
        if K[j][2].startswith(("k_check_final", "k_rho_rescale", "k_aa")):
            last = j
        if K[j][2].startswith("k_setup_gram"):
            break
        j += 1
    if last is None:
        i += 1
        continue
    t_end = max(k[1] for k in K[i:last + 1])
    nxt = last + 1
    seg = []                                            # kernels up to the next k_global
    while nxt + len(seg) < len(K) and not K[nxt + len(seg)][2].startswith("k_global"):
        seg.append(K[nxt + len(seg)])
    hv = [k for k in seg if k[2].startswith("k_harvest")]
    if not seg:
        break
    # harvest start -> first kernel of the next iteration, over the whole interval up to the next check
    w_end = nxt
    while w_end < len(K) and not K[w_end][2].startswith("k_zero_check"):
        w_end += 1
    hk = [k for k in K[nxt:w_end] if k[2].startswith(HARV_ONLY)]
    itk = [k for k in K[nxt:w_end] if k[2].startswith(ITER)]
    if hk and itk:
        h0 = min(k[0] for k in hk)
        (hs_sync if hv else hs_async).append(itk[0][0] - h0)
        if not hv:
            a_kern.append(max(k[1] for k in hk) - h0)
    if not hv:
        bubble.append(seg[0][0] - t_end)
    else:
        t_hv = hv[0][1]
        before = [k for k in seg if k[0] < t_hv and k[2].startswith(HARV)]
        gram = [k for k in seg if k[2].startswith("k_setup_gram")]
        setup = [k for k in seg if k[2] == "k_setup"]
        after = [k for k in seg if k[0] >= t_hv and not k[2].startswith(("k_setup", "k_harvest"))]
        h_gap1.append(before[0][0] - t_end)
        h_kern.append(t_hv - before[0][0])
        if gram:
            h_gram.append(gram[0][1] - gram[0][0])
        if setup:
            h_gap2.append(setup[0][0] - t_hv); h_setup.append(setup[0][1] - setup[0][0]); h_total.append(setup[0][1] - t_end)
            t_done = setup[0][1]
        else:
            h_total.append(t_hv - t_end); t_done = t_hv
        if after:
            h_next.append(after[0][0] - t_done)
    i = last + 1
L = []


def line(name, v):
    v = us(v)
    if len(v):
        L.append(f"  {name:58s} n {len(v):4d}  median {np.median(v):8.1f} us  mean {v.mean():8.1f}  max {v.max():8.0f}  total {v.sum() / 1e3:7.1f} ms")


L.append("checks without a harvest:")
line("last check kernel end -> first kernel of the next iteration", bubble)
L.append("checks with a harvest:")
line("last check kernel end -> first harvest kernel", h_gap1)
line("harvest kernels (first start -> k_harvest end)", h_kern)
line("k_harvest end -> k_setup start", h_gap2)
line("k_setup", h_setup)
line("k_setup_gram (beside the harvest kernels)", h_gram)
line("last check kernel end -> k_setup end (k_harvest end without refill)", h_total)
line("then -> first kernel of the next iteration", h_next)
L.append("harvest start -> first kernel of the next iteration:")
line("synchronous harvests", hs_sync)
line("asynchronous harvests (k_harvest ends after the next k_global starts)", hs_async)
line("asynchronous harvests: first start -> last end, beside the interval", a_kern)
L.append("kernels of the path:")
for nm in ("k_setup", "k_setup_gram", "k_check_build", "k_cone_sub<2>", "k_cone<true>", "k_state_save", "k_harvest"):
    line(nm, [k[1] - k[0] for k in K if k[2] == nm or (nm.endswith(">") and k[2].startswith(nm))])
txt = "\n".join(L) + "\n"
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write(txt)
print(txt, end="")
