"""Restatement of the bond-singlet pairing estimator of the t-J model, an independent dense pair operator, and the candidate rule of
the device's pair slice as a pure function.

Basis: |S> = product of c+ over the occupied sites in row-major order; t-J states 0 = up, 1 = down, 2 = empty.  For a nearest-neighbour
bond with i the left / upper and j the right / lower site,
    Delta+_ij = (c+_i,up c+_j,down - c+_i,down c+_j,up) / sqrt(2),        Delta_ij = (Delta+_ij)+.
Local estimators (square_tJ_model.h:569-602) with rho(S') = jw psi(S') / psi(S), psi the graded row-major amplitude and
jw = (-1)^(electrons strictly between i and j in row-major order):
    (empty, empty)  delta_dag = conj(rho(up, down) - rho(down, up)) / sqrt(2),  delta = 0
    (up, down)      delta = conj(rho(empty, empty)) / sqrt(2),                   delta_dag = 0
    (down, up)      delta = -conj(rho(empty, empty)) / sqrt(2),                  delta_dag = 0
    anything else   both 0
and the registry value of the bond is (conj(delta_dag) + delta) / 2: its |psi|^2-weighted mean over all configurations is
<Psi|Delta_ij|Psi> / <Psi|Psi>.

The local path: inside a row (column) pass the two sites of a horizontal (vertical) bond are adjacent in the row-major (column-major)
mode order, and psi' / psi is the ratio of two contractions of the sign-decorated network, ReplaceNNSiteTrace / Trace.  The decoration
leaves out Sigma = (-1)^(nf (nf + 1) / 2), which a move that changes the electron number nf by +-2 flips:
    rho = -ReplaceNNSiteTrace / Trace                     in both passes (the column pass's ratio carries jw by itself).
"""
import numpy as np

UP_, DN_, EMPTY = 0, 1, 2
SQ2 = np.sqrt(2.0)


def nn_bonds(rows, cols):
    """(key, (r1, c1), (r2, c2)) of every nearest-neighbour bond, "h" bonds first"""
    for r in range(rows):
        for c in range(cols - 1):
            yield "h", (r, c), (r, c + 1)
    for r in range(rows - 1):
        for c in range(cols):
            yield "v", (r, c), (r + 1, c)


def pair_candidates(c1, c2):
    """the configurations of the pair a pair operator connects (c1, c2) to: slot 0 and slot 1, None for "no candidate" """
    if (c1, c2) == (EMPTY, EMPTY):
        return [(UP_, DN_), (DN_, UP_)]
    if (c1, c2) in ((UP_, DN_), (DN_, UP_)):
        return [(EMPTY, EMPTY), None]
    return [None, None]


def tj_pair_table():
    """pair_candidates as the table [3 * 3][2][2] of pepsgpu_nn_pair_slice_fermion ((-1, -1) for none)"""
    tab = -np.ones((9, 2, 2), dtype=np.int32)
    for a in range(3):
        for b in range(3):
            for k, cand in enumerate(pair_candidates(a, b)):
                if cand is not None:
                    tab[a * 3 + b, k] = cand
    return tab


def bond_sc_from_pairs(c1, c2, rho0, rho1):
    """(delta_dag, delta) of one bond from the ratios rho of its two candidate slots"""
    if (c1, c2) == (EMPTY, EMPTY):
        return np.conj(rho0 - rho1) / SQ2, 0.0
    if (c1, c2) == (UP_, DN_):
        return 0.0, np.conj(rho0) / SQ2
    if (c1, c2) == (DN_, UP_):
        return 0.0, -np.conj(rho0) / SQ2
    return 0.0, 0.0


def registry_value(delta_dag, delta):
    return (np.conj(delta_dag) + delta) / 2


def jw_between(cfg, s1, s2):
    """(-1)^(electrons strictly between the two sites in row-major order)"""
    cfg = np.asarray(cfg)
    cols = cfg.shape[1]
    ia, ib = sorted((s1[0] * cols + s1[1], s2[0] * cols + s2[1]))
    return (-1) ** int(np.sum(cfg.ravel()[ia + 1:ib] != EMPTY))


def sc_from_amplitudes(cfg, amp):
    """the registry value of every bond of one configuration from fresh amplitudes: amp(configuration) -> psi.
    Returns ({"h": [rows][cols - 1], "v": [rows - 1][cols]}, number of non-zero pair terms)"""
    cfg = np.asarray(cfg)
    rows, cols = cfg.shape
    out = {"h": np.zeros((rows, cols - 1), complex), "v": np.zeros((rows - 1, cols), complex)}
    psi0, terms = amp(cfg), 0
    for key, s1, s2 in nn_bonds(rows, cols):
        rho = [0.0, 0.0]
        for k, cand in enumerate(pair_candidates(int(cfg[s1]), int(cfg[s2]))):
            if cand is None:
                continue
            new = cfg.copy()
            new[s1], new[s2] = cand
            rho[k] = jw_between(cfg, s1, s2) * amp(new) / psi0
            terms += 1
        out[key][s1] = registry_value(*bond_sc_from_pairs(int(cfg[s1]), int(cfg[s2]), rho[0], rho[1]))
    return out, terms


# ---- the dense operator, built from single annihilation operators (no Jordan-Wigner string formula of a PAIR is used) ----
def _annihilate(s, site, spin):
    """c_{site, spin} on the basis state s (tuple of site states): (sign, new state) or None.  c+ stand in row-major order, so moving
    c_site to its c+ passes one operator per occupied site before it."""
    if s[site] != spin:
        return None
    sign = (-1) ** sum(1 for q in s[:site] if q != EMPTY)
    new = list(s)
    new[site] = EMPTY
    return sign, tuple(new)


def dense_delta(rows, cols, i, j):
    """<S'|Delta_ij|S> in the basis of tj_nnn_ref.all_tj_configs (index = base-3 number of the row-major configuration), i < j flat
    sites: Delta_ij = (c_j,down c_i,up - c_j,up c_i,down) / sqrt(2)"""
    import itertools
    n = rows * cols
    pw = 3 ** np.arange(n - 1, -1, -1)
    M = np.zeros((3 ** n, 3 ** n))
    for idx, s in enumerate(itertools.product((UP_, DN_, EMPTY), repeat=n)):
        for coef, spin_i, spin_j in ((1.0, UP_, DN_), (-1.0, DN_, UP_)):
            first = _annihilate(s, i, spin_i)
            if first is None:
                continue
            second = _annihilate(first[1], j, spin_j)
            if second is None:
                continue
            M[int(np.array(second[1]) @ pw), idx] += coef * first[0] * second[0] / SQ2
    return M


# ---- the candidate rule of pair_cand_kernel / the host layer's PairTable as a pure function ----
def pair_cand_rule(e1, e2, order, nf, pair_table):
    """extended states (state + d * variant) of the two sites of a bond under candidate k, and Sigma(S') / Sigma(S):
    returns (cand [2][2], sign [2]).  order 0: row-major (variant = parity of the electrons up to and including the site), 1:
    column-major (variant = 2 + parity of the electrons strictly before the site).  No candidate: the own states and sign 0."""
    nf = np.asarray(nf) % 2
    d = len(nf)
    tab = np.asarray(pair_table).reshape(d * d, 2, 2)
    a, b, v1 = e1 % d, e2 % d, e1 // d
    before = (v1 & 1) ^ int(nf[a]) if order == 0 else (v1 & 1)
    cand, sign = np.zeros((2, 2), dtype=np.int32), np.zeros(2, dtype=np.int32)
    for k in range(2):
        pa, pb = (int(x) for x in tab[a * d + b, k])
        if pa < 0:
            cand[k] = (e1, e2)
            continue
        na, nb = int(nf[pa]), int(nf[pb])
        if order == 0:
            cand[k] = (pa + d * (before ^ na), pb + d * (before ^ na ^ nb))
        else:
            cand[k] = (pa + d * (2 + before), pb + d * (2 + (before ^ na)))
        sign[k] = 1 if na + nb == int(nf[a]) + int(nf[b]) else -1
    return cand, sign


# ---- the local path on the oracle ----
def local_pair_ratios(fs, cfg, trun_para):
    """ReplaceNNSiteTrace / Trace (the RAW ratio of decorated contractions, no sign applied) of every pair candidate of one
    configuration inside the oracle's row pass (horizontal bonds) and column pass (vertical bonds): {(key, s1, k): ratio}"""
    from oracle.bmps import LEFT, DOWN, RIGHT, UP, HORIZONTAL, VERTICAL
    from oracle.fermion import ROW, COL
    cfg = np.asarray(cfg)
    rows, cols = cfg.shape
    out = {}
    for key, s1, s2 in nn_bonds(rows, cols):
        cands = pair_candidates(int(cfg[s1]), int(cfg[s2]))
        if cands[0] is None:
            continue
        order, orient = (ROW, HORIZONTAL) if key == "h" else (COL, VERTICAL)
        comp = fs.component(cfg, order, trun_para)
        tn, c = comp.tn, comp.contractor
        if key == "h":
            c.GenerateBMPSApproach(tn, UP)
            for _ in range(s1[0]):
                c.ShiftBMPSWindow(tn, DOWN)
            c.InitBTen(tn, LEFT, s1[0])
            c.GrowFullBTen(tn, RIGHT, s1[0], 1, True)
            for _ in range(s1[1]):
                c.ShiftBTenWindow(tn, RIGHT)
        else:
            c.GenerateBMPSApproach(tn, LEFT)
            for _ in range(s1[1]):
                c.ShiftBMPSWindow(tn, RIGHT)
            c.InitBTen(tn, UP, s1[1])
            c.GrowFullBTen(tn, DOWN, s1[1], 2, True)
            for _ in range(s1[0]):
                c.ShiftBTenWindow(tn, DOWN)
        psi = c.Trace(tn, s1, orient)
        for k, cand in enumerate(cands):
            if cand is None:
                continue
            new = cfg.copy()
            new[s1], new[s2] = cand
            ne = fs.ext_config(new, order)
            out[(key, s1, k)] = c.ReplaceNNSiteTrace(tn, s1, s2, orient, fs.ext[s1[0]][s1[1]][ne[s1]], fs.ext[s2[0]][s2[1]][ne[s2]]) / psi
    return out


def sc_from_local_ratios(cfg, ratios, sign=-1.0):
    """the registry value of every bond from the local path's raw ratios; sign = -1 is Sigma(S') / Sigma(S) of a pair move"""
    cfg = np.asarray(cfg)
    rows, cols = cfg.shape
    out = {"h": np.zeros((rows, cols - 1), complex), "v": np.zeros((rows - 1, cols), complex)}
    for key, s1, s2 in nn_bonds(rows, cols):
        rho = [sign * ratios.get((key, s1, k), 0.0) for k in range(2)]
        out[key][s1] = registry_value(*bond_sc_from_pairs(int(cfg[s1]), int(cfg[s2]), rho[0], rho[1]))
    return out
