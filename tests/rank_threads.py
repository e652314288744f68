"""Thread-per-rank runner of the several-rank GPU tests: the ranks are contexts of one process, one host thread each, over
the in-process loopback communicator (lgh_comm.hip, unique id "LGHLOCAL..."), which replaces only the transport - as in
tests/test_gpu_pipeline.py::test_multi_rank_run_on_one_gpu.  No RCCL, no further processes.

Every collective of the library is synchronous on the host over this transport, so a call that contains one (the set-up, a
halo sum, a CG over the ranks) has to be made on every rank at the same time: run_ranks() does that.  The loopback barrier
gives up after 60 s and marks the group broken, so a collective mismatch ends as an error of the ranks that waited, not as
a hang; a thread that is still alive after the time-out fails the test with "a rank did not finish"."""
import os
import threading

TIMEOUT = 150.0


def local_unique_id():
    return (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0")


def run_ranks(n, fn, timeout=TIMEOUT):
    """fn(rank) on n daemon threads at once; the list of results, rank by rank.  An exception on any rank fails the
    caller with all of them."""
    out, err = {}, {}

    def main(rank):
        try:
            out[rank] = fn(rank)
        except BaseException as ex:  # noqa: BLE001 - reported below
            err[rank] = repr(ex)

    threads = [threading.Thread(target=main, args=(r,), daemon=True) for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in threads), "a rank did not finish (collective mismatch?)"
    assert not err, err
    return [out[r] for r in range(n)]


class Ranks:
    """One HydroOperator - hence one Context with owner = prob.owner, lgh_comm_init and lgh_comm_set_neighbors(*prob.neighbors()),
    then the set-up calls, which sum the Jacobi diagonal, the volume and the zone count over the ranks - per rank problem."""

    def __init__(self, probs, **kw):
        from laghos_amd.hydro import HydroOperator
        self.probs, self.n = list(probs), len(probs)
        cid = local_unique_id()
        self.ops = [None] * self.n

        def make(r):
            p = self.probs[r]
            nbr_rank, nbr_nodes = p.neighbors()
            comm = dict(nranks=self.n, rank=r, unique_id=cid, nbr_rank=nbr_rank, nbr_nodes=nbr_nodes)
            self.ops[r] = HydroOperator(p, comm=comm, **kw)
            assert self.ops[r].multi

        try:
            run_ranks(self.n, make)
        except BaseException:
            self.close()
            raise

    def run(self, fn, timeout=TIMEOUT):
        """fn(rank, operator, problem) on every rank at once"""
        return run_ranks(self.n, lambda r: fn(r, self.ops[r], self.probs[r]), timeout)

    def close(self):
        for g in self.ops:
            if g is not None:
                g.close()
        self.ops = [None] * self.n
