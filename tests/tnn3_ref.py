"""Test-side restatement of the reference's three-site exchange updater on the oracle contractor: MCUpdateSquareTNN3SiteUpdateBase
::operator() (square_3site_updater.h:28-91) and MCUpdateSquareTNN3SiteExchange::TNN3SiteUpdateImpl (:109-158), bosonic states, one
std::mt19937 per walker (oracle.vmc.StdMT19937: the long double draw of SuwaTodoStateUpdate = two raw words).  Used by
tests/test_gpu_tnn3.py as the chain the device must reproduce, in the way tests/tgemm_ref.py restates the tensor GEMM."""
import itertools

import numpy as np

from oracle import vmc
from oracle.bmps import DOWN, HORIZONTAL, LEFT, RIGHT, UP, VERTICAL


class MCUpdateSquareTNN3SiteExchange:
    def __init__(self, seed=0):
        self.rng = vmc.StdMT19937(seed)

    def u_longdouble(self):
        return self.rng.u_longdouble()

    def __call__(self, sitps, comp):
        """one sweep (:28-91); returns [accepted / (cols (rows - 2) + rows (cols - 2))]"""
        tn, c = comp.tn, comp.contractor
        accept = 0
        c.SetTruncateParams(comp.trun_para)
        c.GenerateBMPSApproach(tn, UP)
        for row in range(tn.rows):
            c.InitBTen(tn, LEFT, row)
            c.GrowFullBTen(tn, RIGHT, row, 3, True)
            comp.amplitude = c.ReplaceTNNSiteTrace(tn, (row, 0), HORIZONTAL, *[sitps[row][k][int(comp.config[row, k])] for k in range(3)])
            for col in range(tn.cols - 2):
                accept += self.update(((row, col), (row, col + 1), (row, col + 2)), HORIZONTAL, sitps, comp)
                if col < tn.cols - 3:
                    c.ShiftBTenWindow(tn, RIGHT)
            if row < tn.rows - 1:
                c.ShiftBMPSWindow(tn, DOWN)
        c.DeleteInnerBMPS(LEFT)
        c.DeleteInnerBMPS(RIGHT)
        c.GenerateBMPSApproach(tn, LEFT)
        for col in range(tn.cols):
            c.InitBTen(tn, UP, col)
            c.GrowFullBTen(tn, DOWN, col, 3, True)
            comp.amplitude = c.ReplaceTNNSiteTrace(tn, (0, col), VERTICAL, *[sitps[k][col][int(comp.config[k, col])] for k in range(3)])
            for row in range(tn.rows - 2):
                accept += self.update(((row, col), (row + 1, col), (row + 2, col)), VERTICAL, sitps, comp)
                if row < tn.rows - 3:
                    c.ShiftBTenWindow(tn, DOWN)
            if col < tn.cols - 1:
                c.ShiftBMPSWindow(tn, RIGHT)
        c.DeleteInnerBMPS(UP)
        return [accept / (tn.cols * (tn.rows - 2) + tn.rows * (tn.cols - 2))]

    def update(self, sites, bond_dir, sitps, comp):
        """:109-158 for one triple"""
        spins = tuple(int(comp.config[s]) for s in sites)
        if spins[0] == spins[1] == spins[2]:
            return False                                                    # :118, no trace and no draw
        perms = sorted(set(itertools.permutations(sorted(spins))))          # std::next_permutation order of the sorted triple
        init = perms.index(spins)
        psis = []
        for i, p in enumerate(perms):
            if i == init:
                psis.append(comp.amplitude)
            else:
                psis.append(comp.contractor.ReplaceTNNSiteTrace(comp.tn, sites[0], bond_dir,
                                                                *[sitps[s[0]][s[1]][p[k]] for k, s in enumerate(sites)]))
        psi_abs_max = max(abs(x) for x in psis)
        weights = [float(np.real(x / psi_abs_max) ** 2 + np.imag(x / psi_abs_max) ** 2) for x in psis]     # std::norm
        final = vmc.suwa_todo_state_update(init, weights, self.u_longdouble)
        if final == init:
            return False
        comp.UpdateLocal(sitps, psis[final], *[(s, perms[final][k]) for k, s in enumerate(sites)])
        return True
