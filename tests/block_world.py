"""Helpers of the block halo tests: util.EmulatedWorld's routing for block vectors.

P simulated ranks on ONE GPU in the 1-rank context.  A block halo is packed by the GPU block pack kernel
(sgpu_debug_pack_block), routed between the ranks on the host and injected (sgpu_debug_inject_halo_block); the block
applies that follow run k_csr_block with the boundary mask and k_csr_boundary_block on one stream.  The wire layout is
the scalar one with every segment K times as long: segment i of a rank's send buffer is sendCount[i] * K values at
sendDispl[i] * K, and the receive buffer is a block vector over the halo positions."""
import numpy as np

from saena_amd import capi
from tests import util


class BlockWorld(util.EmulatedWorld):
    def exchange_block(self, Xs):
        """Xs[r]: BlockVector holding rank r's slice of the input block"""
        K = Xs[0].K
        sends = []
        for r in range(self.P):
            n = int(self.plans[r][1].sum())
            sends.append(self.g[r].debug_pack_block(Xs[r], n).ravel() if n else np.zeros(0))
        for r in range(self.P):
            sr, sc, sd, rr, rc, rd = self.plans[r]
            recv = np.zeros(int(rc.sum()) * K)
            for q, cnt, dsp in zip(rr, rc, rd):
                qs = self.plans[q]
                k = list(qs[0]).index(r)
                src = sends[q][qs[2][k] * K:(qs[2][k] + qs[1][k]) * K]
                assert len(src) == cnt * K
                recv[dsp * K:(dsp + cnt) * K] = src
            self.g[r].debug_inject_halo_block(recv.reshape(-1, K))

    def slices_block(self, V, split):
        """V: (n, K) host block -> one BlockVector per rank"""
        return [capi.BlockVector(int(split[r + 1] - split[r]), V.shape[1], V[split[r]:split[r + 1]]) for r in range(self.P)]

    def gather_block(self, Ys):
        return np.concatenate([Y.download() for Y in Ys], axis=0)

    def set_block_lanes(self, lanes):
        for G in self.g:
            G.set_block_lanes(lanes)
