"""CPU test of csrc/omc_shor_block.h, the per-block arithmetic of the device evaluator of Shor-mode certificates (k_scert_clean /
k_scert_minor): tests/host/shor_block_check.cpp, a stand-alone program that includes nothing of the project but that header, is built with
the address and undefined-behaviour sanitisers and fed 2000 seeded order-5 blocks of four kinds -- PSD up to rounding (G G' with one
eigenvalue set to +-1e-14 ||G G'||), indefinite, exact zero, and arrow blocks whose V entries are zero.  Its output is compared with numpy:
the smallest eigenvalue, the block minus its negative part, Gamma - E + ||E||_F I and the final shift, each within 50 eps ||block||_F (both
algorithms are backward stable with constants of the order of the dimension).  Largest observed ratio to that bound on the CPU: 0.128
(smallest eigenvalue 0.078, negative part 0.128, spread 0.018, final shift 0.073, block after the shift 0.073)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimalmatrixcompletion.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "shor_block_check.cpp")
NBLOCKS = 2000
EPS = np.finfo(float).eps
TRI = [(r, c) for c in range(5) for r in range(c + 1)]      # packed upper triangle by columns (include/omc.h)
VENT = [(1, 2), (3, 4), (1, 3), (2, 4), (1, 4), (2, 3)]


def pack(G):
    return np.array([G[r, c] for (r, c) in TRI])


def unpack(p):
    G = np.zeros((5, 5))
    for e, (r, c) in enumerate(TRI):
        G[r, c] = G[c, r] = p[e]
    return G


def make_blocks():
    """(kind, block, residuals e12 e34 e13 e24) per block; kinds 0 PSD up to rounding, 1 indefinite, 2 zero, 3 arrow."""
    rng = np.random.default_rng(20250611)
    out = []
    for t in range(NBLOCKS):
        kind = t % 4
        scale = 10.0 ** rng.uniform(-3, 3)
        if kind == 0:
            F = rng.standard_normal((5, 5)) * scale
            Bm = F @ F.T
            w, V = np.linalg.eigh(Bm)
            w[0] = (1e-14 if t % 8 == 0 else -1e-14) * np.linalg.norm(Bm)
            Bm = (V * w) @ V.T
            Bm = 0.5 * (Bm + Bm.T)
            res = rng.uniform(-1, 1, 4) * 0.1 * np.linalg.norm(Bm)
        elif kind == 1:
            Bm = rng.standard_normal((5, 5)) * scale
            Bm = 0.5 * (Bm + Bm.T)
            res = rng.uniform(-1, 1, 4) * 0.1 * np.linalg.norm(Bm)
        elif kind == 2:
            Bm = np.zeros((5, 5)); res = np.zeros(4)
        else:
            Bm = np.diag(rng.uniform(0.0, 1.0, 5)) * scale
            Bm[0, 1:] = Bm[1:, 0] = rng.standard_normal(4) * scale
            res = np.zeros(4)
        out.append((kind, Bm, res))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shor_block") / "shor_block_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I", CSRC, SRC, "-o", exe],
                   check=True)
    return exe


def test_header_is_plain_cpp():
    """omc_shor_block.h includes <math.h> and nothing else: no HIP header, nothing of the project; the qualifiers are behind a macro."""
    text = open(os.path.join(CSRC, "omc_shor_block.h")).read()
    inc = re.findall(r"^\s*#\s*include\s*(\S+)", text, flags=re.M)
    assert inc == ["<math.h>"]
    assert "hip" not in " ".join(inc).lower()


def test_blocks_against_numpy(program):
    blocks = make_blocks()
    lines = [str(len(blocks))]
    for _, Bm, res in blocks:
        lines.append(" ".join(repr(float(v)) for v in list(pack(Bm)) + list(res)))
    got = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=120).stdout.strip().split("\n")
    assert len(got) == len(blocks)
    worst = dict(min_eig=0.0, negative_part=0.0, spread=0.0, final_shift=0.0, shifted_block=0.0)
    nzero_shift = 0
    for (kind, Bm, res), line in zip(blocks, got):
        v = np.array([float(x) for x in line.split()])
        assert v.shape == (48,)
        lo, clean, spread, nrm, sh, final = v[0], unpack(v[1:16]), unpack(v[16:31]), v[31], v[32], unpack(v[33:48])
        tol = 50.0 * EPS * np.linalg.norm(Bm)
        w, V = np.linalg.eigh(Bm)
        E = np.zeros((5, 5))
        e3 = 0.5 * (Bm[1, 4] + Bm[2, 3])
        for (r, c), e in zip(VENT, list(res) + [e3, e3]):
            E[r, c] = E[c, r] = e
        nE = np.sqrt((E * E).sum())
        S = Bm - E + nE * np.eye(5)
        low = np.linalg.eigvalsh(S)[0]
        want_shift = max(-low, 0.0)
        errs = dict(min_eig=abs(lo - w[0]), negative_part=np.abs(clean - (Bm - (V * np.minimum(w, 0.0)) @ V.T)).max(),
                    spread=max(np.abs(spread - S).max(), abs(nrm - nE)), final_shift=abs(sh - want_shift),
                    shifted_block=np.abs(final - (S + want_shift * np.eye(5))).max())
        for key, err in errs.items():
            assert err <= tol, (kind, key, err, tol)
            if tol > 0.0:
                worst[key] = max(worst[key], err / tol)
        if kind == 0:
            # PSD up to rounding: ||E||_F >= 1.118 ||E||_2 (E is trace-free), so the shift of the spread covers a negative part below
            # 0.118 ||E||_F and the further shift is exactly 0
            assert nE > 0.0 and 0.118 * nE > 2e-14 * np.linalg.norm(Bm)
            assert sh == 0.0, (sh, nE)
            nzero_shift += 1
        if kind == 2:
            assert lo == 0.0 and sh == 0.0 and not final.any() and not clean.any()
    print("largest error / (50 eps ||block||_F):", {k: round(x, 4) for k, x in worst.items()})
    assert nzero_shift == NBLOCKS // 4
