#!/usr/bin/env python
"""Re-ranking (models.rerank, poi_rerank) at the Gowalla shape (N = 100 k POIs, dim 128, 200 bins, 50 k users): explicit candidate
lists of 100 / 1000 / 4096 POIs for calls of 1 / 64 / 4096 rows, the plain score (BPR tables) and the spatial score (bins on the fly),
ragged lists (one per row: the model's own top-L candidates, shuffled) and one shared list (L random POIs), every list ordered in full
(k = L).  Beside the fused call, in the same process and on the same rows and lists:
  stages   from the library's event timing over the fused calls: "score_lists" and "rerank_lists", milliseconds per call;
  all      the ranker's compute_sub_candidates(k = L) over ALL POIs: what re-ranking a list saves over ranking the table.  On the
           ragged cells the lists ARE that call's result, so the fused call must return the same ids;
  rows     poi_score_rows + a torch gather of the listed columns + poi_rerank_lists (rows within 1 GiB of scores at a time): the route
           the library offered before - the same bits, so the same ids on every row;
  torch    a float32 yardstick: items[lists] gather, bmm with the rows (plus wd * poi_dist_prob's gathered columns under the spatial
           score), a stable descending sort - the same ids on the rows without near-ties.
Per cell: microseconds per call as the median of --repeats timed windows (min and max alongside) of a fixed number of chained calls -
as many as fill --window-ms - with ONE synchronisation at the end of the window, after a warm-up window; the ratios fused / route of
the medians; the share of rows with the same ids.  Prints one JSON line.
    python tools/bench_rerank.py [--repeats N] [--window-ms T] [--quick]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from poi_amd import data as pdata, harness
from poi_amd.models import _ptr

STAGES = ("score_lists", "rerank_lists")
GIB = 1 << 30


def windows(fn, window_ms, repeats):
    """A window is a FIXED number of chained calls and one synchronisation: the number that fills window_ms at the duration of one
    synchronised call."""
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    calls = max(1, min(10000, int(window_ms / max((time.perf_counter() - t0) * 1e3, 1e-3))))

    def one():
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls
    one()
    v = sorted(one() for _ in range(repeats))
    return dict(us=round(v[len(v) // 2], 2), min=round(v[0], 2), max=round(v[-1], 2), calls=calls)


def stage_times(m, fn, calls=5):
    m.ctx.timing(True)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out = {s: round(m.ctx.timing_get(s)[0] / calls, 4) for s in STAGES}
    m.ctx.timing(False)
    return out


class Cell:
    """The rows and lists of one cell on the device, and the three other routes over them."""

    def __init__(self, m, ids, lists, shared):
        self.m, self.ids, self.shared = m, ids, shared
        row_ids, self.users, lo = m._users_rows(ids)
        self.users = self.users.contiguous()
        self.term = m._rank_term(row_ids, lo)
        self.lists = lists                               # (L) shared / (n, L) ragged, int32 on the device
        self.n, self.L = len(ids), lists.shape[-1]
        self.cols = (lists[None, :].expand(self.n, self.L) if shared else lists).long()
        self.off = None if shared else torch.arange(self.n + 1, device=m.device, dtype=torch.int32) * self.L

    def fused(self):
        return self.m.rerank(self.ids, self.lists, self.L, sync=False)

    def all_pois(self):
        return self.m.compute_sub_candidates(self.ids, self.L, sync=False)

    def rows_route(self):
        m, N = self.m, self.m.n_item
        sc = torch.empty((self.n, self.L), dtype=torch.float32, device=m.device)
        step = max(1, GIB // (4 * N))
        for o in range(0, self.n, step):
            u = self.users[o:o + step]
            term = None if self.term is None else (self.term[0], self.term[1][o:o + step], self.term[2][o:o + step])
            full = torch.empty((u.shape[0], N), dtype=torch.float32, device=m.device)
            m.ctx.check(m.lib.poi_score_rows(m.ctx.handle, *m._tile_operands(u, m._items(), m.kdim, term), _ptr(full), N, m._stream()))
            sc[o:o + step] = full.gather(1, self.cols[o:o + step])
        idx = torch.empty((self.n, self.L), dtype=torch.int32, device=m.device)
        m.ctx.check(m.lib.poi_rerank_lists(m.ctx.handle, _ptr(self.off), _ptr(self.lists), self.n, self.lists.numel(), _ptr(sc), None, 1.0, 0.0, self.L,
                                           _ptr(idx), None, None, None, m._stream()))
        return idx

    def torch_route(self):
        m, N = self.m, self.m.n_item
        items = m._items()[:N].float()
        out = torch.empty((self.n, self.L), dtype=torch.int32, device=m.device)
        step = max(1, GIB // (4 * max(self.L * m.kdim, N if self.term is not None else 1)))
        for o in range(0, self.n, step):
            cols, u = self.cols[o:o + step], self.users[o:o + step]
            sc = torch.bmm(items[cols], u[:, :, None])[:, :, 0]
            if self.term is not None:
                wd, sts, lp = self.term[0], self.term[1][o:o + step].contiguous(), self.term[2][o:o + step].contiguous()
                prob = torch.empty((u.shape[0], N), dtype=torch.float32, device=m.device)
                m.ctx.check(m.lib.poi_dist_prob(m.ctx.handle, _ptr(m.coords), _ptr(m._cphi), _ptr(m._binthr), _ptr(lp), _ptr(sts), u.shape[0], N, m.n_dist,
                                                m.dd * 1000.0, _ptr(prob), m._stream()))
                sc = sc + wd.reshape(-1)[0] * prob.gather(1, cols)
            order = torch.sort(sc, dim=1, descending=True, stable=True)[1]
            out[o:o + step] = cols.gather(1, order).int()
        return out


def same_rows(a, b):
    return round(float((a == b).all(dim=1).float().mean()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--quick", action="store_true", help="4 k users / 10 k POIs, 3 windows of 30 ms")
    a = ap.parse_args()
    U, N, D = (4096, 10000, 128) if a.quick else (50000, 100000, 128)
    if a.quick:
        a.repeats, a.window_ms = 3, 30.0
    ds = pdata.make_synthetic(U, N, 20, seed=1, dd=200, ud_km=40, local=0.8)
    out = dict(shape=dict(users=U, pois=N, dim=D), cells=[])
    rng = np.random.default_rng(3)
    for spatial in (False, True):
        p = harness.default_params()
        p.update(latent_size=D, gru=2 if spatial else 0)
        m = harness.build_model(ds, p, seed=5)
        m.update_trained_items()
        if spatial:
            m.update_trained_dists()
            m.update_trained_users(torch.rand((U, D), device=m.device) - 0.5)
            m.update_trained_sus(torch.rand((U, m.n_dist + 1), device=m.device))
        else:
            m.update_trained_users()
        score = "geo" if spatial else "plain"
        for n in (1, 64, 4096):
            ids = rng.choice(U, n, replace=False).astype(np.int64)
            for L in (100, 1000, 4096):
                own = m.compute_sub_candidates(ids, L)
                perm = torch.argsort(torch.rand((n, L), device=m.device), dim=1)
                for shared in (False, True):
                    lists = torch.as_tensor(rng.choice(N, L, replace=False).astype(np.int32)).to(m.device) if shared else own.gather(1, perm).contiguous()
                    C = Cell(m, ids, lists, shared)
                    got = C.fused()
                    cell = dict(score=score, n_rows=n, list=L, layout="shared" if shared else "ragged", lists_path=m.ctx.last_plan("lists_path"))
                    cell["same_ids"] = dict(rows=same_rows(got, C.rows_route()), torch=same_rows(got, C.torch_route()))
                    if not shared:
                        cell["same_ids"]["all"] = same_rows(got, own)
                    assert cell["same_ids"]["rows"] == 1.0, cell
                    cell["fused"] = windows(C.fused, a.window_ms, a.repeats)
                    cell["stages_ms"] = stage_times(m, C.fused)
                    for name, fn in (("all", C.all_pois), ("rows", C.rows_route), ("torch", C.torch_route)):
                        cell[name] = windows(fn, a.window_ms, a.repeats)
                        cell["ratio_" + name] = round(cell["fused"]["us"] / cell[name]["us"], 3)
                    print("[bench_rerank] %s rows %d list %d %s: fused %.1f us (score %.3f ms, sort %.3f ms), all POIs %.1f us, rows + gather %.1f us, "
                          "torch %.1f us, same ids %s" % (score, n, L, cell["layout"], cell["fused"]["us"], cell["stages_ms"]["score_lists"],
                                                          cell["stages_ms"]["rerank_lists"], cell["all"]["us"], cell["rows"]["us"], cell["torch"]["us"],
                                                          cell["same_ids"]), file=sys.stderr, flush=True)
                    out["cells"].append(cell)
                    del C
        assert m.ctx.take_bad_ids() == 0
        del m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
