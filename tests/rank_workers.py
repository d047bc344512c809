"""W ranks on the one GPU of the test box, started ONCE per (test module, world): every rank runs the same ordered list of named
cases in lock-step and the parent gets, per case and rank, the case's result or a traceback.  A plain helper module (no fixture, no
pytest setting): tests/test_gpu_ranks_small.py builds its module-scoped fixtures on `run_world`.

A case is a function `case(env)` of the test module, listed by name in the module's dict CASES; it runs on every rank with the same
arguments and RETURNS what the parent is to judge (numpy arrays, numbers, tuples) -- it asserts nothing, so an exception in a case
is a finding of its own.  `env` (RankEnv) gives the rank, the world and `env.context(...)`: a fresh api.Context with the
collectives of dist.TorchCollectives set (gloo between the processes, staged through the host) and option fit_persistent = 1 --
several processes cannot keep persistent grids co-resident on one GPU, so the ranks use the launch-per-iteration fit
(tests/test_gpu_two_ranks.py gives the same reason).

How a run ends by itself, whatever a rank does:
  * the process group has a timeout (GROUP_TIMEOUT_S): a rank left alone in an exchange gets an error from the hook, hence
    CGE_E_COLLECTIVE from the library, hence a traceback in its record -- nothing waits on the GPU, the waiting is the host's;
  * between two cases the ranks meet at a multiprocessing barrier (not a collective of the group, which a diverged case may have
    left in any state) with a timeout beyond the group's; a rank that raised still goes there.  Behind the barrier every rank
    reads every rank's verdict: all returned or all raised -- the next case runs; MIXED -- the ranks diverged, every rank stops
    and the remaining cases are recorded as not run, naming the case that diverged;
  * the parent's queue reads and joins have timeouts, and whatever is still alive afterwards is terminated.
So a diverged rank is a failed test that names its case, not a stuck run."""
import os
import queue as queue_mod
import socket
import sys
import time
import traceback

GROUP_TIMEOUT_S = 60  # of every collective of the process group
BARRIER_TIMEOUT_S = GROUP_TIMEOUT_S + 45  # a rank that raised at once waits here for the ranks that run into the group's timeout
START_TIMEOUT_S = 180  # W interpreters importing torch side by side
JOIN_TIMEOUT_S = 20


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class RankEnv:
    def __init__(self, rank, world):
        self.rank, self.world = rank, world
        self._open = []

    def context(self, capacity_doubles=1 << 16, ext=False, options=()):
        """A fresh context with the collectives set FIRST (the uploads themselves may be split), then `options` in order, then
        fit_persistent = 1.  Returns (ctx, coll)."""
        import torch
        from cge.jl_amd import api
        from cge.jl_amd.dist import TorchCollectives

        ctx = api.Context(0)
        self._open.append(ctx)
        coll = TorchCollectives(ctx, int(capacity_doubles), torch.device("cuda", 0), ext=ext)
        for key, value in options:
            ctx.set_option(key, value)
        ctx.set_option("fit_persistent", 1)
        return ctx, coll

    def close_all(self):
        for ctx in self._open:
            try:
                ctx.close()
            except Exception:
                pass
        self._open = []


def _worker(rank, world, port, module_name, case_names, sys_path, q, barrier, verdicts):
    t0 = time.perf_counter()
    try:
        for p in reversed(sys_path):
            if p not in sys.path:
                sys.path.insert(0, p)
        import datetime
        import importlib

        import torch
        import torch.distributed as dist

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=GROUP_TIMEOUT_S))
        torch.cuda.set_device(0)
        mod = importlib.import_module(module_name)
        env = RankEnv(rank, world)
        env.context()  # (the first context pays for the runtime's start: part of the start-up, not of a case)
        env.close_all()
        q.put((rank, "__ready__", "ok", time.perf_counter() - t0))
    except Exception:
        q.put((rank, "__ready__", "error", traceback.format_exc()))
        q.put((rank, "__done__", "ok", None))
        return
    stopped_by = None
    for name in case_names:
        if stopped_by is not None:
            q.put((rank, name, "error", f"not run: the ranks diverged in case {stopped_by!r}"))
            continue
        t1 = time.perf_counter()
        try:
            out = mod.CASES[name](env)
            record = (rank, name, "ok", (out, time.perf_counter() - t1))
            verdicts[rank] = 1
        except Exception:
            record = (rank, name, "error", traceback.format_exc())
            verdicts[rank] = 2
        env.close_all()
        q.put(record)
        try:
            barrier.wait(BARRIER_TIMEOUT_S)  # every verdict of this case is written ...
            mixed = len(set(verdicts[:])) > 1
            barrier.wait(BARRIER_TIMEOUT_S)  # ... and read, before the next case overwrites it
        except Exception:  # (a broken barrier: a rank never came)
            mixed = True
        if mixed:
            stopped_by = name
    q.put((rank, "__done__", "ok", None))
    try:
        if stopped_by is None and dist.is_initialized():
            dist.destroy_process_group()
    except Exception:
        pass


class WorldRun:
    """records[case][rank] = ("ok", result) or ("error", text); startup_s: the wall time from the first start() to the last rank's
    first context; cases_s[case]: the slowest rank's time in the case; total_s: the whole run."""

    def __init__(self, world):
        self.world = world
        self.records, self.cases_s = {}, {}
        self.startup_s = self.total_s = float("nan")

    def results(self, case):
        """The per-rank results of a case, rank order; an AssertionError that carries the traceback(s) otherwise."""
        rec = self.records.get(case, {})
        bad = [f"rank {r}: {rec[r][1] if r in rec else 'no record (the rank ended or was terminated before it)'}"
               for r in range(self.world) if r not in rec or rec[r][0] != "ok"]
        assert not bad, f"case {case!r} on {self.world} ranks:\n" + "\n".join(bad)
        return [rec[r][1] for r in range(self.world)]


def run_world(world, module_name, case_names, budget_s=420):
    """Spawn `world` ranks, run the cases, collect.  Never raises for what a rank did; always returns within about budget_s."""
    import torch.multiprocessing as mp

    assert 2 <= world <= 5  # (with the parent: far below the limit on processes that hold the GPU)
    mpc = mp.get_context("spawn")
    q, barrier, verdicts = mpc.Queue(), mpc.Barrier(world), mpc.Array("i", world)
    port = _free_port()
    run = WorldRun(world)
    t0 = time.perf_counter()
    procs = [mpc.Process(target=_worker, args=(r, world, port, module_name, list(case_names), list(sys.path), q, barrier, verdicts),
                         daemon=True) for r in range(world)]
    for p in procs:
        p.start()
    ready, done = 0, 0
    deadline = t0 + budget_s
    while done < world:
        limit = min(deadline, t0 + START_TIMEOUT_S) if ready < world else deadline
        left = limit - time.perf_counter()
        if left <= 0:
            break
        try:
            rank, name, status, payload = q.get(timeout=min(left, 5.0))
        except queue_mod.Empty:
            if not any(p.is_alive() for p in procs) and q.empty():
                break
            continue
        if name == "__ready__":
            ready += 1
            if status != "ok":
                run.records.setdefault("__ready__", {})[rank] = (status, payload)
            if ready == world:
                run.startup_s = time.perf_counter() - t0
        elif name == "__done__":
            done += 1
        else:
            if status == "ok":
                out, secs = payload
                run.cases_s[name] = max(run.cases_s.get(name, 0.0), secs)
                payload = out
            run.records.setdefault(name, {})[rank] = (status, payload)
    for p in procs:
        p.join(JOIN_TIMEOUT_S if done == world else 1)
    for p in procs:
        if p.is_alive():
            p.terminate()
    for p in procs:
        p.join(JOIN_TIMEOUT_S)
        if p.is_alive():
            p.kill()
    run.total_s = time.perf_counter() - t0
    if "__ready__" in run.records:  # a rank that never started: every case names it
        text = "; ".join(f"rank {r}: {v[1]}" for r, v in sorted(run.records["__ready__"].items()))
        for name in case_names:
            for r in range(world):
                run.records.setdefault(name, {}).setdefault(r, ("error", "the ranks did not start: " + text))
    return run
