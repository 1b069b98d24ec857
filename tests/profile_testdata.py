"""
The yardstick of the profile (PSSM) tests (tests/test_profile_alignment_cpu.py, tests/test_profile_alignment_gpu.py):
`definition`, Gotoh's three tables as a plain numpy double loop over the positions of the row (i) and of the profile (j),
all (profile, row) pairs at once, one result rule per mode; and `brute_force`, the worded definitions of
tests/local_testdata.py, tests/semiglobal_testdata.py and tests/fit_testdata.py read with a profile's positions for the
symbols of y.  Nothing under prograph_amd/ imports this file, and it imports nothing from there.
"""
import numpy as np

import fit_testdata
import local_testdata
import semiglobal_testdata
from local_testdata import lengths

NEG = -(1 << 29)                 # -inf for int32 tables: 2048 steps of 255 below it and any score above it stay in range
MODES = ("local", "semiglobal", "fit")
_BRUTE = {"local": local_testdata.brute_force, "semiglobal": semiglobal_testdata.brute_force, "fit": fit_testdata.brute_force}


def definition(mode, P_list, gap, gap_open, X):
    """(Q, N) int64 scores of the profiles `P_list` ((L_q, A) integer arrays; all L_q positions count) against the rows of
    X (a row without its trailing zeros; an interior 0 is symbol 0), i over the row and j over the profile:
        E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
        H[i][j] = max(H[i-1][j-1] + P[j][x_i], E[i][j], F[i][j])   (local: and 0),   E[0][j] = F[i][0] = -inf, H[i][0] = 0,
        local:       H[0][j] = 0,            s = max over i <= len x, j <= L of H[i][j]
        semiglobal:  H[0][j] = 0,            s = max(max over i <= len x of H[i][L], max over j <= L of H[len x][j])
        fit:         H[0][j] = -(o + j e),   s = max over i <= len x of H[i][L]
    The tables are filled to the longest row and profile; a cell reads lower i and j only, so the cells beyond a pair's own
    lengths feed nothing that is read.  Row i - 1 gives E and the diagonal term for every j at once; the loop over j
    carries F and H along the row."""
    assert mode in MODES
    X = np.atleast_2d(np.asarray(X, dtype=np.intp))
    P_list = [np.asarray(p, dtype=np.int64) for p in P_list]
    lx, ly = lengths(X), np.array([len(p) for p in P_list], dtype=np.int64)
    LX, LY, Q, N, e, o = int(lx.max(initial=0)), int(ly.max()), len(P_list), len(X), int(gap), int(gap_open)
    Pp = np.zeros((LY, Q, P_list[0].shape[1]), dtype=np.int32)   # [j][q][a], zeros past a profile's length
    for q, p in enumerate(P_list):
        Pp[:len(p), q] = p
    H = np.zeros((LY + 1, Q, N), dtype=np.int32)                  # row i - 1, then row i
    if mode == "fit":
        H[1:] = -(o + e * np.arange(1, LY + 1, dtype=np.int32))[:, None, None]    # all of the profile is paid for
    E = np.full((LY + 1, Q, N), NEG, dtype=np.int32)
    Hn, A, T = np.zeros_like(H), np.empty_like(H[1:]), np.empty_like(H[1:])  # row i, and two rows of scratch
    at = np.broadcast_to(ly[None, :, None], (1, Q, N))
    inside = np.arange(LY + 1)[:, None, None] <= ly[None, :, None]           # j <= L
    best = np.take_along_axis(H, at, 0)[0].copy()                 # H[0][L]: 0, or -(o + L e)
    for i in range(1, LX + 1):
        np.subtract(H[1:], o + e, out=T)
        np.subtract(E[1:], e, out=E[1:])
        np.maximum(E[1:], T, out=E[1:])                           # E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e)
        np.add(H[:-1], Pp[:, :, X[:, i - 1]], out=A)
        np.maximum(A, E[1:], out=A)                               # the aligned pair H[i-1][j-1] + P[j][x_i] | x_i unaligned
        if mode == "local":
            np.maximum(A, 0, out=A)
        F = np.full((Q, N), NEG, dtype=np.int32)                  # F[i][0] = -inf; Hn[0] = H[i][0] = 0
        for j in range(1, LY + 1):
            F = np.maximum(F - e, Hn[j - 1] - (o + e))
            np.maximum(A[j - 1], F, out=Hn[j])
        H, Hn = Hn, H                                             # row 0 of either buffer is never written
        live = (i <= lx)[None, :]
        if mode == "local":
            best = np.where(live, np.maximum(best, np.where(inside, H, 0).max(0)), best)
            continue
        best = np.where(live, np.maximum(best, np.take_along_axis(H, at, 0)[0]), best)        # H[i][L]
        if mode == "semiglobal" and (i == lx).any():
            best = np.where((i == lx)[None, :], np.maximum(best, np.where(inside, H, NEG).max(0)), best)   # row len x
    return best.astype(np.int64)


def brute_force(mode, P, gap, gap_open, x):
    """The worded definition of the mode (every stretch choice it allows, every alignment path walked to its end) for one
    profile and one token list: the y of the sequence tests is the list of the profile's positions, and the table they
    index as S[x_i][y_j] is the profile turned round, T[a][j] = P[j][a]."""
    P = np.asarray(P, dtype=np.int64)
    return _BRUTE[mode](P.T, int(gap), int(gap_open), list(x), list(range(len(P))))


def random_profile(rng, length, a, lo=-6, hi=9):
    """An (length, a) profile with random entries per position in lo..hi - not derivable from any table - whose largest
    entry is exactly hi."""
    P = rng.integers(lo, hi + 1, (length, a))
    P[rng.integers(0, length), rng.integers(0, a)] = hi
    return P
