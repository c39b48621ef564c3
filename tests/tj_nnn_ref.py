"""Restatement of the reference's diagonal-hop hooks on the oracle's amplitudes, and an independent dense Hamiltonian.

EvaluateNNNEnergy of the two fermionic models returns -t2 ComplexConjugate(psi_ex / psi) for a diagonal, or 0:
  square_spinless_fermion.h:178-212  0 when config1 == config2 (:188), "one site empty, the other site filled" otherwise (:190);
  square_tJ_model.h:424-463          0 when config1 == config2 or NEITHER site is empty (:437-442): an electron hops into a hole,
                                     an up and a down spin never exchange along a diagonal.
The reference's graded ReplaceNNNSiteTrace carries the Jordan-Wigner sign in the tensor algebra; on the oracle's amplitudes (fresh
FermionSITPS.amplitude of the hopped configuration, parity legs row-major) the sign is explicit: jw = (-1)^(fermions strictly
between the two ends in row-major order).  oracle/fermion.py:187-201 has this form for the spinless model only -- its skip rule
(cfg[a] == cfg[b]) would exchange up and down spins in a t-J state -- hence this file.

The dense Hamiltonian is built without any of the above: basis |S> = product of c+ over the occupied sites in row-major order; a hop
between two sites carries (-1)^(occupied sites strictly between them); the spin exchange moves no fermion past another and is sign-free.
"""
import itertools

import numpy as np

UP_, DN_, EMPTY = 0, 1, 2           # vmc_basic/tj_single_site_state.h:19-23


def tj_state(rows, cols, D, seed=12, weight_seed=4):
    """a random parity-even t-J state as tests/test_gpu_energy_slices.py:276-279 builds one: the occupied component of the spinless
    generator twice, differently weighted (0 up, 1 down: odd; 2 empty)"""
    from peps_amd import fermion
    base = fermion.random_even_state(rows, cols, D, seed=seed)
    rng = np.random.default_rng(weight_seed)
    return fermion.FermionState([[[t[0], t[0] * rng.uniform(0.5, 1.5, size=t[0].shape), t[1]] for t in row] for row in base.tensors],
                                base.par, [1, 1, 0])


def oracle_view(state):
    """oracle.fermion.FermionSITPS of a peps_amd.fermion.FermionState (as tests/test_gpu_fermion.py::_oracle_view)"""
    from oracle import fermion as ofermion
    from oracle.graded import GT
    gts = [[[GT(state.tensors[r][c][s][..., None], list(state.par[r][c]) + [np.array([int(state.nf[s])])], [-1, 1, 1, -1, -1])
             for s in range(state.d)] for c in range(state.cols)] for r in range(state.rows)]
    return ofermion.FermionSITPS(gts)


def diagonals(rows, cols):
    """(key, a, b) of every plaquette diagonal: "dr" (r, c) <-> (r+1, c+1), "ur" (r+1, c) <-> (r, c+1)"""
    for r in range(rows - 1):
        for c in range(cols - 1):
            yield "dr", (r, c), (r + 1, c + 1)
            yield "ur", (r + 1, c), (r, c + 1)


def hop_allowed(model, c1, c2):
    if c1 == c2:                                                # square_spinless_fermion.h:188, square_tJ_model.h:437
        return False
    if model == "tj" and c1 != EMPTY and c2 != EMPTY:           # square_tJ_model.h:438-439
        return False
    return True


def nnn_energy(fs, cfg, trun_para, t2, model, bonds=None, psi0=None):
    """sum over the diagonals of EvaluateNNNEnergy on the oracle's amplitudes; returns (energy, number of allowed diagonals).
    bonds: optional dict that receives "dr" / "ur" [rows - 1][cols - 1]"""
    cfg = np.asarray(cfg)
    rows, cols = cfg.shape
    occ = np.array(fs.nf)[cfg].ravel()
    if psi0 is None:
        psi0 = fs.amplitude(cfg, trun_para)
    if bonds is not None:
        bonds.update(dr=np.zeros((rows - 1, cols - 1), complex), ur=np.zeros((rows - 1, cols - 1), complex))
    e, count = 0.0, 0
    for key, a, b in diagonals(rows, cols):
        if not hop_allowed(model, int(cfg[a]), int(cfg[b])):
            continue
        count += 1
        ia, ib = sorted((a[0] * cols + a[1], b[0] * cols + b[1]))
        jw = (-1) ** int(np.sum(occ[ia + 1:ib]))
        new = cfg.copy()
        new[a], new[b] = cfg[b], cfg[a]
        eb = -t2 * jw * np.conj(fs.amplitude(new, trun_para) / psi0)      # square_tJ_model.h:461-462, square_spinless_fermion.h:210-211
        e += eb
        if bonds is not None:
            bonds[key][min(a[0], b[0]), a[1]] = eb
    return e, count


def tj_local_energy(fs, cfg, trun_para, t, t2, J, V, mu, bonds=None):
    """E_loc of the t-t'-J-V model: the oracle's nearest-neighbour part (SquaretJVModelOBC with t2 = 0) + the restated diagonal hops"""
    from oracle import fermion as ofermion
    e_nn = ofermion.SquaretJVModelOBC(t, 0.0, J, V, mu).CalEnergy(fs, cfg, trun_para)[0]
    e_nnn, count = nnn_energy(fs, cfg, trun_para, t2, "tj", bonds)
    return e_nn + e_nnn, count


def all_tj_configs(rows, cols):
    return np.array(list(itertools.product((UP_, DN_, EMPTY), repeat=rows * cols)), dtype=np.int64).reshape(-1, rows, cols)


def dense_ttj_hamiltonian(rows, cols, t, t2, J, V, mu):
    """<S'|H|S> of H = -t sum_<ij>,s (c+_is c_js + h.c.) - t2 sum_<<ij>>,s (...) + J sum_<ij> (S_i.S_j - n_i n_j / 4) + V sum_<ij> n_i n_j
    - mu N on the no-double-occupancy space, in the basis of all_tj_configs (index = base-3 number of the row-major configuration)."""
    n = rows * cols
    dim = 3 ** n
    pw = 3 ** np.arange(n - 1, -1, -1)
    H = np.zeros((dim, dim))
    nn = [(r * cols + c, r * cols + c + 1) for r in range(rows) for c in range(cols - 1)] + \
         [(r * cols + c, (r + 1) * cols + c) for r in range(rows - 1) for c in range(cols)]
    nnn = [(r * cols + c, (r + 1) * cols + c + 1) for r in range(rows - 1) for c in range(cols - 1)] + \
          [(r * cols + c + 1, (r + 1) * cols + c) for r in range(rows - 1) for c in range(cols - 1)]
    for idx, s in enumerate(itertools.product((UP_, DN_, EMPTY), repeat=n)):
        s = np.array(s)
        occ = s != EMPTY
        H[idx, idx] += -mu * occ.sum()
        for amp, links in ((-t, nn), (-t2, nnn)):
            for i, j in links:
                if occ[i] != occ[j]:                                          # an electron and a hole: the electron hops
                    new = s.copy()
                    new[i], new[j] = s[j], s[i]
                    H[int(new @ pw), idx] += amp * (-1) ** int(occ[i + 1:j].sum())
        for i, j in nn:
            if occ[i] and occ[j]:
                H[idx, idx] += V
                if s[i] != s[j]:
                    H[idx, idx] += -0.5 * J                                   # Sz Sz - 1/4
                    new = s.copy()
                    new[i], new[j] = s[j], s[i]
                    H[int(new @ pw), idx] += 0.5 * J                          # (S+ S- + S- S+) / 2: no fermion passes another
    return H


def rayleigh(H, psi):
    psi = np.asarray(psi)
    return (np.conj(psi) @ (H @ psi)) / (np.conj(psi) @ psi)
