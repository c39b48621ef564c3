"""Restatement of the singlet-pair correlation SC_singlet_pair_corr of the t-J models (model_solvers/base/
singlet_pair_correlation_measurement_mixin.h): the index mapping (:136-245), the local estimator (:501-508) from fresh amplitudes, the
excited-state propagation (:349-534) on the oracle's BMPSWalker, and an independent dense operator.

Basis and pair operator as tests/pair_ref.py: |S> = product of c+ over the occupied sites in row-major order, t-J states 0 = up,
1 = down, 2 = empty, Delta+_ij = (c+_i,up c+_j,down - c+_i,down c+_j,up) / sqrt(2) with i the left site of a horizontal bond.

For the reference bond (y1, x1)-(y1, x1 + 1) and the target bond (y2, x2)-(y2, x2 + 1), y2 > y1, the local estimator of S is non-zero
only for an (empty, empty) reference bond and an (up, down) or (down, up) target bond:
    value = 1/2 conj(rho_ud - rho_du) * (+1 for (up, down), -1 for (down, up)),
    rho_x = psi(S with ref -> x, target -> (empty, empty)) / psi(S).
Both bonds are adjacent pairs in row-major order and pair operators are even: no Jordan-Wigner string.

The walker path: a fermionic amplitude is Sigma(N_f) times an ordinary contraction of decorated components, and a pair move on two
adjacent modes changes the components of its two sites only.  The excited row carries Sigma(S') / Sigma(S) = -1 (two electrons in), the
target replacement -1 again (two electrons out): the RAW two-site traces of the excited walkers over the raw trace of the original
walker are rho itself.
"""
import numpy as np

import pair_ref

UP_, DN_, EMPTY = 0, 1, 2


# ---- the index mapping (:136-245) ----
def valid_ref_bonds(Ly, Lx, ref_bonds=()):
    """the reference bonds measured, in output order: all of them row by row, or the selection without its out-of-lattice members,
    sorted by (y, x) (:193-212; a selection is NOT de-duplicated there)"""
    if Ly < 2 or Lx < 2:
        return []
    if len(ref_bonds) == 0:
        return [(y, x) for y in range(Ly - 1) for x in range(Lx - 1)]
    return sorted((int(y), int(x)) for y, x in ref_bonds if 0 <= y < Ly - 1 and 0 <= x < Lx - 1)


def num_sc_pairs(Ly, Lx, ref_bonds=()):
    return sum((Ly - 1 - y) * (Lx - 1) for y, _ in valid_ref_bonds(Ly, Lx, ref_bonds))


def index_mapping(Ly, Lx, ref_bonds=()):
    """[(ref_y, ref_x, 0, tgt_y, tgt_x, 0)] in output order"""
    return [(y1, x1, 0, y2, x2, 0) for y1, x1 in valid_ref_bonds(Ly, Lx, ref_bonds) for y2 in range(y1 + 1, Ly) for x2 in range(Lx - 1)]


def coord_string(Ly, Lx, ref_bonds=()):
    lines = ["# idx ref_y ref_x ref_orient tgt_y tgt_x tgt_orient"]
    lines += ["%d %d %d %d %d %d %d" % ((i,) + m) for i, m in enumerate(index_mapping(Ly, Lx, ref_bonds))]
    return "\n".join(lines) + "\n"


# ---- the dense operator ----
def dense_pair_corr(rows, cols, ref, tgt, cache=None):
    """<S'|Delta+_ref Delta_tgt|S> as a product of pair_ref.dense_delta matrices (built from single c / c+); ref, tgt = (y, x) of the
    left site"""
    cache = {} if cache is None else cache
    mats = []
    for y, x in (ref, tgt):
        i = y * cols + x
        if i not in cache:
            cache[i] = pair_ref.dense_delta(rows, cols, i, i + 1)
        mats.append(cache[i])
    return mats[0].T @ mats[1]


# ---- the estimator from fresh amplitudes ----
def estimator_from_amplitudes(cfg, amp, ref_bonds=(), du_sign=-1.0, conj=True):
    """the value of every bond pair of one configuration in mapping order, amp(configuration) -> psi.  du_sign and conj exist so that
    a test can show the wrong conventions miss.  Returns (values, number of non-zero terms)"""
    cfg = np.asarray(cfg)
    Ly, Lx = cfg.shape
    out = np.zeros(num_sc_pairs(Ly, Lx, ref_bonds), dtype=complex)
    psi0, terms = None, 0
    for i, (y1, x1, _, y2, x2, _) in enumerate(index_mapping(Ly, Lx, ref_bonds)):
        if cfg[y1, x1] != EMPTY or cfg[y1, x1 + 1] != EMPTY:
            continue
        tgt = (int(cfg[y2, x2]), int(cfg[y2, x2 + 1]))
        if tgt not in ((UP_, DN_), (DN_, UP_)):
            continue
        if psi0 is None:
            psi0 = amp(cfg)
        rho = []
        for pair in ((UP_, DN_), (DN_, UP_)):
            new = cfg.copy()
            new[y1, x1], new[y1, x1 + 1] = pair
            new[y2, x2], new[y2, x2 + 1] = EMPTY, EMPTY
            rho.append(amp(new) / psi0)
        v = 0.5 * (rho[0] - rho[1]) * (1.0 if tgt == (UP_, DN_) else du_sign)
        out[i] = np.conj(v) if conj else v
        terms += 1
    return out, terms


# ---- the excited-state propagation on the oracle's BMPSWalker ----
def walker_estimator(fs, cfg, trun_para, ref_bonds=()):
    """MeasureSingletPairCorrelation (:349-534) for one configuration on oracle.fermion.FermionSITPS: extended states of the changed
    pairs from pair_ref.pair_cand_rule, RAW two-site traces, rho = (-1)(-1) excited / original.  The schedule is the reference's: two
    excited walkers and one original walker per reference bond, forked from up_stack[y1], evolved row by row, scanned left to right
    per target row.  Returns (values in mapping order, number of non-zero terms)"""
    from oracle.bmps import DOWN, RIGHT, UP
    from oracle.contractor import BMPSWalker
    from oracle.fermion import ROW
    cfg = np.asarray(cfg)
    Ly, Lx = cfg.shape
    table = pair_ref.tj_pair_table()
    comp = fs.component(cfg, ROW, trun_para)
    tn, c = comp.tn, comp.contractor
    ext = fs.ext_config(cfg, ROW)
    c.GenerateBMPSApproach(tn, UP)
    c.GrowFullBMPS(tn, UP)
    up_stack, down_stack = c.bmps_set[UP], c.bmps_set[DOWN]
    assert len(down_stack) == Ly and len(up_stack) == Ly
    out, terms = [], 0
    for y1, x1 in valid_ref_bonds(Ly, Lx, ref_bonds):
        ref_valid = cfg[y1, x1] == EMPTY and cfg[y1, x1 + 1] == EMPTY
        cand, sign = pair_ref.pair_cand_rule(int(ext[y1, x1]), int(ext[y1, x1 + 1]), 0, fs.nf, table)
        walkers = []
        for k in range(2):                                   # slot 0: (up, down) injected, slot 1: (down, up)
            mpo = tn.get_row(y1)
            if ref_valid:
                assert sign[k] == -1
                mpo[x1], mpo[x1 + 1] = fs.ext[y1][x1][cand[k][0]], fs.ext[y1][x1 + 1][cand[k][1]]
            w = BMPSWalker(tn, up_stack[y1], UP, y1, trun_para)
            w.Evolve(mpo)
            walkers.append(w)
        orig = BMPSWalker(tn, up_stack[y1], UP, y1, trun_para)
        orig.Evolve(tn.get_row(y1))
        walkers.append(orig)
        absorbed = y1 + 1
        for y2 in range(y1 + 1, Ly):
            bottom = down_stack[Ly - 1 - y2]
            while absorbed < y2:
                for w in walkers:
                    w.Evolve(tn.get_row(absorbed))
                absorbed += 1
            mpo = tn.get_row(y2)
            for w in walkers:
                w.InitBTenLeft(mpo, bottom, 0)
                w.InitBTenRight(mpo, bottom, 1)
            for x2 in range(Lx - 1):
                tgt = (int(cfg[y2, x2]), int(cfg[y2, x2 + 1]))
                val = 0.0
                if ref_valid and tgt in ((UP_, DN_), (DN_, UP_)):
                    tc, ts = pair_ref.pair_cand_rule(int(ext[y2, x2]), int(ext[y2, x2 + 1]), 0, fs.nf, table)
                    assert ts[0] == -1 and ts[1] == 0
                    a, b = fs.ext[y2][x2][tc[0][0]], fs.ext[y2][x2 + 1][tc[0][1]]
                    psi = orig.TraceWithTwoSiteBTen(mpo[x2], mpo[x2 + 1], x2, mpo, bottom)
                    rho = [sign[k] * ts[0] * walkers[k].TraceWithTwoSiteBTen(a, b, x2, mpo, bottom) / psi for k in range(2)]
                    val = 0.5 * np.conj(rho[0] - rho[1]) * (1.0 if tgt == (UP_, DN_) else -1.0)
                    terms += 1
                out.append(val)
                if x2 < Lx - 2:
                    for w in walkers:
                        w.ShiftBTenWindow(mpo, bottom, RIGHT)
            for w in walkers:
                w.ClearBTen()
    return np.array(out, dtype=complex), terms
