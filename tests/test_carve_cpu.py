"""CPU test of csrc/omc_carve.h and csrc/omc_walks.h, the one definition from which the host API both sizes and carves its packed device
buffers.  tests/host/carve_check.cpp, a stand-alone program that reads the HIP headers for their types only, is built with the address and
undefined-behaviour sanitisers; for every line of dimensions it runs each walk over a measuring Carve and then over a host allocation of
exactly the measured size, writes every array end to end and prints the totals and, in walk order, the offset of every pointer the walk
filled with the alignment of its type.  Asserted here: the two passes agree; the arrays start in walk order at distinct, aligned offsets
inside the buffer (an array ends where the next begins, so none overlaps); the adjacencies that code outside the walks relies on, which fix
the widths those callers assume; the 32-byte rows of the evaluators' matrices; the evaluator's totals against
omc_shor_dual_bound_plan; and that no buffer is larger than the expression that sized it before the walks existed (restated below)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimalmatrixcompletion.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "carve_check.cpp")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")

# stage S N n m k nnz rmax Rmax shor keep accel      (S slots, N nodes of the capacity; Rmax at least 1 + k (k + 1) / 2)
STAGE = [
    (1, 1, 4, 5, 1, 7, 1, 2, 0, 0, 0),              # one slot, rank 1, rmax 1, Rmax at its minimum, nothing kept
    (1, 1, 12, 14, 8, 60, 1, 37, 0, 1, 1),          # rank 8 with Rmax at its minimum, certificates kept, acceleration on
    (3, 7, 24, 30, 2, 250, 5, 14, 0, 1, 0),         # omc_relax_reserve: room for 4 more nodes than staged
    (4, 4, 12, 14, 1, 60, 3, 8, 1, 1, 0),           # Shor mode with its certificates kept (no Lam)
    (2, 5, 520, 530, 1, 9000, 4, 11, 0, 0, 0),      # np16 > 512, reserve
    (256, 300, 100, 100, 2, 3000, 6, 20, 0, 1, 1),
]
# shor S N nq1 m nm      (nq1 = max(nq, 1): the first line is nq = 0)
SHOR = [(1, 1, 1, 5, 20), (4, 9, 152, 14, 168), (3, 3, 7, 530, 520 * 530)]
# dual V n k nnz Rmax rmax Lmax
DUAL = [(1, 4, 1, 7, 2, 1, 1), (3, 12, 8, 60, 37, 1, 1), (2, 520, 1, 9000, 11, 4, 2), (5, 100, 2, 3000, 20, 6, 3)]
# project B NP
PROJECT = [(1, 16), (3, 528), (2, 1040)]
# scert B V n m nnz Rmax rmax Lmax nqs nmb nv1max nv2max slab store_clean: small corners here, the shapes of the plan test further down
SCERT = [(1, 1, 4, 5, 7, 2, 1, 1, 0, 0, 0, 0, 0, 0), (2, 3, 12, 14, 60, 8, 3, 2, 7, 1, 9, 11, 0, 1), (2, 2, 150, 150, 900, 5, 2, 1, 300, 2, 600, 600, 22500, 0)]
# the shapes tests/test_shor_dual_bound_cpu.py plans: n m B nq_stride max_cuts box_rows
PLAN_SHAPES = [(12, 14, 3, 152, 2, 0), (200, 200, 1, 632732, 0, 5)]


def plan_cases(omc):
    """(shape, sanitise, V, plan) for both sanitise values and V = B, V = 2 B, with the worst case of the call's lists: nqmax = nq_stride and
    two keys per minor on each side."""
    out = []
    for (n, m, B, nqs, cuts, box) in PLAN_SHAPES:
        for sanitise in (False, True):
            plan = omc.pkg.api.shor_dual_bound_plan(n, m, 1, B, nqs, max_cuts=cuts, nonstandard_box_rows=box, sanitise=sanitise)
            for V in (B, 2 * B):
                out.append(((n, m, B, nqs, cuts, box), sanitise, V, plan))
    return out


def scert_line(shape, sanitise, V, plan):
    n, m, B, nqs, cuts, box = shape
    nmb = -(-nqs // 256)
    return (B, V, n, m, n * m // 3, plan["Rmax"], plan["rmax"], max(cuts, 1), nqs, nmb, 2 * nqs, 2 * nqs, plan["slab_doubles"], int(sanitise))


def parse(text):
    cases, cur, walk = [], None, None
    for ln in text.splitlines():
        t = ln.split()
        if t[0] == "case":
            cur = dict(kind=t[1], dims=tuple(int(x) for x in t[2:]), walks={})
            cases.append(cur)
        elif t[0] == "walk":
            walk = dict(measure=int(t[2]), place=int(t[3]), fields={}, order=[])
            cur["walks"][t[1]] = walk
        elif t[0] == "field":
            walk["fields"][t[1].split(".")[-1]] = int(t[2])
            walk["order"].append((int(t[2]), int(t[3])))
    return cases


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("carve") / "carve_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I", HIP_INCLUDE, "-I", os.path.join(ROOT, "include"), "-I", CSRC, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def report(program, omc):
    """Every dimension set through the program, once for the whole module."""
    lines = [("stage",) + d for d in STAGE] + [("shor",) + d for d in SHOR] + [("dual",) + d for d in DUAL] + [("project",) + d for d in PROJECT]
    lines += [("scert",) + d for d in SCERT] + [("scert",) + scert_line(*c) for c in plan_cases(omc)]
    text = "".join(" ".join(str(x) for x in ln) + "\n" for ln in lines)
    got = subprocess.run([program], input=text, capture_output=True, text=True, timeout=300)
    assert got.returncode == 0, got.stderr[-2000:]
    cases = parse(got.stdout)
    assert len(cases) == len(lines)
    return cases


def of_kind(report, kind):
    return [c for c in report if c["kind"] == kind]


def test_carve_header_is_plain_cpp():
    """omc_carve.h includes standard headers and nothing else: no HIP header, nothing of the project."""
    inc = re.findall(r"^\s*#\s*include\s*(\S+)", open(os.path.join(CSRC, "omc_carve.h")).read(), flags=re.M)
    assert inc and all(i.startswith("<") for i in inc)
    assert "hip" not in " ".join(inc).lower()


def test_passes_agree_and_arrays_are_in_order_aligned_and_inside_the_buffer(report):
    """An array runs from its pointer to the next pointer of the walk (or to the walk's end), so arrays that start in walk order at
    non-decreasing offsets cannot overlap; two pointers share an offset only where an array is empty (no Lam in Shor mode, an end marker)."""
    nwalks = 0
    for c in report:
        for name, w in c["walks"].items():
            where = (c["kind"], c["dims"], name)
            assert w["measure"] == w["place"], where
            assert len(w["order"]) == len(w["fields"]), where      # no name printed twice
            prev = 0
            for (off, align) in w["order"]:
                assert off >= 0 and off % align == 0, where
                assert prev <= off <= w["measure"], where
                prev = off
            assert w["order"][0][0] == 0, where      # the first array starts the buffer
            nwalks += 1
    assert nwalks >= 100


def test_named_adjacencies(report):
    for c in of_kind(report, "stage"):
        S, N, n, m, k = c["dims"][:5]
        f = c["walks"]["slot_ints"]["fields"]
        assert f["ws_need"] == f["done"] + 4 * S            # one copy of S + 1 ints from done brings both back (the solve loop's check)
        w = c["walks"]["check"]
        f = w["fields"]
        assert f["stamps"] == f["chk_scratch"] + 8 * S * n * k
        assert w["measure"] - f["stamps"] == 8 * (32 + 8 * S)      # the last array: zeroed from stamps to the end
        f = c["walks"]["slot_map"]["fields"]
        assert (f["node_of"], f["init"], f["fin"]) == (0, 4 * S, 8 * S)
    for c in of_kind(report, "shor"):
        f = c["walks"]["shor_fro"]["fields"]
        assert f["trB"] == f["fro2B"] + 8 * c["dims"][0]
    for c in of_kind(report, "dual") + of_kind(report, "scert"):
        V = c["dims"][0] if c["kind"] == "dual" else c["dims"][1]
        n = c["dims"][1] if c["kind"] == "dual" else c["dims"][2]
        NP = (n + 15) // 16 * 16
        pre = c["kind"]
        f = c["walks"][pre + "_ints"]["fields"]      # the zeroed block: 7 ints per view, in this order
        assert [f[x] - f["done"] for x in ("vvalidC", "sweeps", "mw_stat", "zero_end")] == [4 * V, 8 * V, 12 * V, 28 * V]
        f = c["walks"][pre + "_doubles"]["fields"]   # read back with one copy
        assert [f[x] - f["c0"] for x in ("cpen", "cst", "fro2c", "evsum", "scalars_end")] == [8 * V * q for q in range(1, 6)]
        f = c["walks"]["dual_matrices" if pre == "dual" else "scert_doubles"]["fields"]      # zeroed with one memset from MbufC to Mchk
        assert f["VrowC"] == f["MbufC"] + 8 * V * NP * NP and f["Mchk"] == f["VrowC"] + 8 * V * NP * NP
    for c in of_kind(report, "project"):
        B = c["dims"][0]
        f = c["walks"]["project_ints"]["fields"]
        assert [f[x] - f["done"] for x in ("vvalid", "sweeps", "mw_stat", "ints_end")] == [4 * B, 8 * B, 12 * B, 28 * B]


def test_evaluator_matrix_rows_are_32_byte_aligned(report):
    """The multi-workgroup eigen-kernels read MbufC / VrowC / Mchk in 32-byte rows: every piece starts on a multiple of 32 bytes."""
    seen_unaligned_head = False
    for c in of_kind(report, "dual") + of_kind(report, "scert"):
        w = c["walks"]["dual_matrices" if c["kind"] == "dual" else "scert_doubles"]
        for x in ("MbufC", "VrowC", "Mchk"):
            assert w["fields"][x] % 32 == 0, (c["dims"], x)
        if c["kind"] == "scert":
            f = w["fields"]      # colmu (V m doubles) is the array in front of MbufC
            seen_unaligned_head = seen_unaligned_head or (f["colmu"] + 8 * c["dims"][1] * c["dims"][3]) % 32 != 0
    assert seen_unaligned_head      # at least one case in which the alignment had something to do


def test_evaluator_totals_within_the_plan(report, omc):
    """The walks of omc_shor_dual_bound_batch plus the index structures of the lists stay within B node_bytes + V view_bytes of
    omc_shor_dual_bound_plan, + 32 for the alignment of the matrices; and within bytes_total + 32 whenever V <= ways * B, which is every
    call the library can make (a node has one view, or two with sanitise).  This departs from the wording that asks for bytes_total + 32
    at both sanitise values and both V = B and V = 2 B: without sanitise the plan counts one view per node, so V = 2 B there is a call the
    library cannot make and bytes_total cannot bound it; those two of the eight cases are held to the per-view bound only.
    The dimensions are the test's own worst case for a stride of nq_stride, not read from the library: every list as long as the stride,
    two distinct keys per minor on each side (nv1max = nv2max = 2 nq_stride, the most a minor can add), a third of the entries observed
    (nnz sizes nothing in these walks), and for the lists what the plan's formula documents per node (`lists`)."""
    by_dims = {c["dims"]: c for c in of_kind(report, "scert")}
    checked = 0
    for (shape, sanitise, V, plan) in plan_cases(omc):
        n, m, B, nqs, cuts, box = shape
        c = by_dims[scert_line(shape, sanitise, V, plan)]
        lists = B * (4 * (20 * nqs + n * m + m + 3) + ((n * m + m + 15) & ~15) + 120)
        total = c["walks"]["scert_doubles"]["measure"] + c["walks"]["scert_ints"]["measure"] + lists
        assert total <= B * plan["node_bytes"] + V * plan["view_bytes"] + 32, (shape, sanitise, V)
        if V <= plan["ways"] * B:
            assert total <= plan["bytes_total"] + 32, (shape, sanitise, V)
            checked += 1
    assert checked == 6


def test_no_buffer_is_larger_than_before(report):
    """Each walk's total against the expression that sized the buffer before the walks (the parent's formula, restated)."""
    for c in of_kind(report, "stage"):
        S, N, n, m, k, nnz, rmax, Rmax, shor, keep, accel = c["dims"]
        per = (0 if shor else nnz) + Rmax + (rmax + k) ** 2
        want = dict(gap=2 * S * 8, small_cone=S * (4 * rmax * k + 3 * k * k) * 8, objcol=S * m * 2 * 8, check=S * n * k * 8 + (32 + 8 * S) * 8,
                    scalars=S * 16 * 8, slot_ints=S * 10 * 4, slot_map=S * 3 * 4, sub_doubles=S * (17 + 256) * 8, sub_ints=S * 15 * 4,
                    subC_doubles=S * 18 * 8, subC_ints=S * 3 * 4, aa_ints=S * 6 * 4, out_scalars=N * 5 * 8, out_ints=N * 2 * 4,
                    cert_slot=S * (2 + per) * 8, cert_flags=S * 2 * 4, cert_node=N * (1 + per) * 8)
        assert set(c["walks"]) == set(want) - (set() if accel else {"aa_ints"}) - (set() if keep else {"cert_slot", "cert_flags", "cert_node"})
        for name, w in c["walks"].items():
            assert w["measure"] <= want[name], (c["dims"], name)
    for c in of_kind(report, "shor"):
        S, N, nq1, m, nm = c["dims"]
        per = 15 * nq1 + m + 2 * nm
        want = dict(shor_fro=S * 2 * 8, shor_cert_slot=S * per * 8, shor_cert_node=N * per * 8, shor_sub_ints=S * 12 * 4)
        for name, w in c["walks"].items():
            assert w["measure"] <= want[name], (c["dims"], name)
    for c in of_kind(report, "dual"):
        V, n, k, nnz, Rmax, rmax, Lmax = c["dims"]
        NP, nn4, ps = (n + 15) // 16 * 16, (n * n + 3) // 4 * 4, (rmax + k) ** 2
        dcount = V * (Rmax * k + Rmax + Lmax * n + n * rmax) + V * (nnz + Rmax + ps + n * rmax) + V * n * k + 5 * V
        want = dict(dual_matrices=V * (2 * NP * NP + nn4) * 8, dual_doubles=dcount * 8, dual_ints=V * (2 + 4 * Rmax + 3 + 4) * 4)
        for name, w in c["walks"].items():
            assert w["measure"] <= want[name], (c["dims"], name)
    for c in of_kind(report, "scert"):
        B, V, n, m, nnz, Rmax, rmax, Lmax, nqs, nmb, nv1, nv2, slab, clean = c["dims"]
        NP, nn4, ps, nm = (n + 15) // 16 * 16, (n * n + 3) // 4 * 4, (rmax + 1) ** 2, n * m
        dcount = B * (1 + 15 * nqs + m + 2 * nm) + B * ((15 * nqs if clean else 0) + nmb) + V * (nv1 + nv2 + 8 * nqs + 2 * nmb + nm + 2 * m) \
            + V * (2 * NP * NP + nn4 + slab) + V * (2 * Rmax + Lmax * n + n * rmax) + V * (Rmax + ps + n * rmax + n + 5) + 4
        icount = B + 2 * V + V * m + V * (2 + 4 * Rmax + 7)
        assert c["walks"]["scert_doubles"]["measure"] <= dcount * 8, c["dims"]
        assert c["walks"]["scert_ints"]["measure"] <= icount * 4, c["dims"]
    for c in of_kind(report, "project"):
        B, NP = c["dims"]
        assert c["walks"]["project_doubles"]["measure"] <= B * (1 + NP) * 8 and c["walks"]["project_ints"]["measure"] <= B * 7 * 4
