"""POI2Vec, CPU half: the float64 oracle step against torch autograd of the reference graph (public/POI2Vec.py:127-177 with the padded bidx
and set_subtensor's last-wins assignment), the loader and the region tree (public/Load_Data_Poi2vec.py) by properties and one tree worked
by hand, the factorised scoring against the literal form, and the declarations (additive to ABI 9)."""
import os
import re

import numpy as np
import pytest

import poi_amd
from poi_amd import data as D
from tests import poi2vec_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = os.path.join(ROOT, "tests", "golden", "sequences_small.txt")


def _tree(rng, n_item, theta=0.5, box=4.0):
    coords = np.stack([rng.uniform(10, 10 + box, n_item), rng.uniform(-60, -60 + box, n_item)], 1)
    coords[0], coords[1] = (10, -60), (10 + box, -60 + box)
    return D.poi2vec_region_tree(coords, theta)


def _tables(rng, n_user, n_item, n_node, dim, scale=0.5):
    return dict(xu=rng.uniform(-scale, scale, (n_user, dim)), wl=rng.uniform(-scale, scale, (n_item, dim)),
                pb=rng.uniform(-scale, scale, (n_node, dim)))


def _autograd_step(P, T, u, targets, contexts, alpha, lam, len_max):
    """The reference's graph: tidx / cidx padded with n_item, wl extended by the zero row, pb = self.pb[bidx] over the PADDED bidx
    (len_max, 4, depth) as one differentiable tensor, the cost over the first L positions; wl and xu[u] by the full gradient, pb by
    assigning sub - alpha grad(sub) occurrence by occurrence in flattened order (the last write wins)."""
    import torch
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    n_item, L = len(P["wl"]), len(targets)
    wl = t64(P["wl"]).requires_grad_()
    xu = t64(P["xu"][u]).requires_grad_()
    tidx = np.concatenate([np.asarray(targets, np.int64), np.full(len_max - L, n_item, np.int64)])
    bidx = T["routes"][tidx].astype(np.int64)                                   # (len_max, 4, depth)
    pb = t64(P["pb"])[torch.as_tensor(bidx)].clone().requires_grad_()
    lrs = t64(T["lrs"][tidx].astype(np.float64))
    probs = t64(T["probs"][tidx].astype(np.float64))
    wlx = torch.cat([wl, torch.zeros(1, wl.shape[1], dtype=torch.float64)])
    cmax = max([len(c) for c in contexts] + [1])
    cidx = np.full((L, cmax), n_item, np.int64)
    for i, c in enumerate(contexts):
        cidx[i, :len(c)] = c
    s = wl @ xu
    plu = torch.exp(s - s.max()) / torch.exp(s - s.max()).sum()                 # softmax() of POI2Vec.py:183-186 on a vector
    cl = wlx[torch.as_tensor(cidx)].sum(dim=1).reshape(L, 1, 1, -1)
    ind = torch.ceil(torch.abs(cl.mean(dim=3))).detach()
    br = torch.sigmoid((pb[:L] * cl).sum(dim=3) * lrs[:L]) * ind
    path = br.prod(dim=2) * probs[:L]
    paths = path.sum(dim=1)
    paths = torch.floor(1 - paths).detach() + paths
    upq = -torch.sum(torch.log(plu[torch.as_tensor(np.asarray(targets, np.int64))] * paths)) / L
    cost = upq + 0.5 * lam * ((xu ** 2).sum() + (wl ** 2).sum())
    cost.backward()
    out = {k: np.array(v, np.float64) for k, v in P.items()}
    out["wl"] = (wl - alpha * wl.grad).detach().numpy()
    out["xu"][u] = (xu - alpha * xu.grad).detach().numpy()
    new = (pb - alpha * pb.grad).detach().numpy().reshape(-1, pb.shape[-1])
    for k, n in enumerate(bidx.reshape(-1)):
        out["pb"][n] = new[k]
    return out, float(upq.detach())


def _case(name):
    rng = np.random.default_rng(17)
    n_item, dim = 60, 12
    T = _tree(rng, n_item)
    P = _tables(rng, 4, n_item, T["n_node"], dim)
    lens = [5, 9, 3, 9]
    data = {}
    for u, L in enumerate(lens):
        data[u] = (rng.integers(0, n_item, L), [rng.integers(0, n_item, rng.integers(1, 5)) for _ in range(L)])
    four = [j for j in range(n_item) if len({tuple(r) for r in T["routes"][j].tolist()}) == 4]      # POIs whose square meets 4 leaves
    data[0][0][2], data[1][0][-1] = four[0], four[1]          # (a duplicate route has probs 0: its write, if last, moves nothing)
    u = 0
    if name == "longest":
        u = 1
    elif name == "empty_context":
        data[0][1][2] = np.zeros(0, np.int64)
    elif name == "repeated_target":
        data[0][0][3] = data[0][0][1]
    elif name == "context_holds_target":
        data[0][1][1] = np.append(data[0][1][1], data[0][0][1])
    elif name == "ind_two":
        k = data[0][1][2]
        P["wl"][k] = 0.45 + 0.004 * np.arange(dim)[None, :]
        data[0][1][2] = np.concatenate([k, k, k])
    return P, T, u, data, max(lens)


@pytest.mark.parametrize("name", ["padding", "longest", "empty_context", "repeated_target", "context_holds_target", "ind_two"])
def test_oracle_step_equals_autograd(name):
    P, T, u, data, len_max = _case(name)
    F = O.forward_terms(P, T, u, *data[u])
    if name == "ind_two":
        assert F["ind"][2] >= 2
    if name == "empty_context":
        assert F["ind"][2] == 0 and F["paths"][2] == 1.0
    with np.errstate(all="ignore"):
        Q, loss = O.step(P, T, u, *data[u], 0.01, 0.001, len_max)
        R, los = _autograd_step(P, T, u, *data[u], 0.01, 0.001, len_max)
    # float64 round-off of a logsumexp / softmax over n_item terms: n_item eps64 max|value| (values: the tables, |.| <= ~1.5 here)
    n_item = len(P["wl"])
    bound = n_item * np.finfo(np.float64).eps * max(1.0, max(np.abs(v).max() for v in P.values()), abs(los) if np.isfinite(los) else 1.0)
    assert np.isfinite(los) and np.isfinite(loss)            # every case, ind_two included, is a parity case
    assert abs(loss - los) <= bound, (loss, los)
    for k in ("xu", "wl", "pb"):
        np.testing.assert_allclose(Q[k], R[k], rtol=0, atol=bound, err_msg=k)
    if name == "padding":                                   # L < len_max: routes[0]'s nodes are written back last
        keep = np.unique(T["routes"][0])
        np.testing.assert_array_equal(Q["pb"][keep], P["pb"][keep])
        assert np.abs(Q["pb"] - P["pb"]).max() > 0
    if name == "longest":
        assert np.abs(Q["pb"][0] - P["pb"][0]).max() > 0     # the root moves


def test_batch_rule_of_one_user_is_the_step_and_rejects():
    P, T, u, data, len_max = _case("padding")
    Q, loss = O.step(P, T, 0, *data[0], 0.01, 0.001, len_max)
    data[7] = (np.zeros(0, np.int64), [])
    R, losses, M = O.batch_step(P, T, [0, 9, -1], data, 0.01, 0.001, len_max, cap=1.0, absmass=True)
    assert losses[0] == loss and np.isnan(losses[1]) and np.isnan(losses[2])
    for k in P:
        np.testing.assert_array_equal(R[k], Q[k])
        assert np.all(M[k] >= np.abs(R[k] - P[k]) - 1e-15)
    # two users at cap 1: wl moves by half the sum; at cap 2 by the sum
    R1, _ = O.batch_step(P, T, [0, 1], data, 0.01, 0.001, len_max, cap=1.0)
    R2, _ = O.batch_step(P, T, [0, 1], data, 0.01, 0.001, len_max, cap=2.0)
    np.testing.assert_allclose(2 * (R1["wl"] - P["wl"]), R2["wl"] - P["wl"], rtol=1e-12, atol=1e-15)
    np.testing.assert_array_equal(R1["xu"][[0, 1]], R2["xu"][[0, 1]])


def test_hand_worked_tree():
    """POIs A = (0, 0), B = (1, 0.5), C = (0.25, 0.25), theta = 0.2.  Root 0: lat [0, 1] x lon [0, 0.5]; latitude is the longer side and
    1 > 0.4: children 1 (lat [0, 0.5]) and 2 (lat [0.5, 1]).  Node 1: 0.5 is not > 0.5, so longitude splits (0.5 > 0.4): children 3 (upper
    half, lon [0.25, 0.5]) and 4 (lon [0, 0.25]).  Node 3: latitude 0.5 > 0.25 and > 0.4: children 5 (lat [0, 0.25]) and 6 (lat [0.25,
    0.5]), both leaves (longitude 0.25 is not > 0.4).  Node 4: children 7, 8.  Then the right half: node 2 -> 9 (lon [0.25, 0.5]), 10; 9 ->
    11, 12; 10 -> 13, 14.  15 nodes, 8 leaves, depth 4.
    A: every corner (+-0.1, +-0.1) goes left at 0 (0.5 < lat is false: +1), right at 1 (node 3's lower edge 0.25 > lon: -1), left at 4
    (0.25 < lat false: +1): route [7, 4, 1, 0], lrs [1, 1, -1, 1], one distinct route: probs (1, 0, 0, 0).
    B: corners (0.9 | 1.1, 0.4 | 0.6): right at 0, left at 2 (0.25 > lon false), right at 9 (0.75 < lat): [12, 9, 2, 0], lrs [1, -1, 1, -1].
    C: corners (0.15, 0.15) -> 7, (0.15, 0.35) -> 5, (0.35, 0.15) -> 8, (0.35, 0.35) -> 6; each leaf overlaps C's square by 0.1 x 0.1:
    probs (0.25, 0.25, 0.25, 0.25)."""
    t = D.poi2vec_region_tree(np.array([[0.0, 0.0], [1.0, 0.5], [0.25, 0.25]]), 0.2)
    assert (t["n_node"], t["n_leaf"], t["depth"]) == (15, 8, 4)
    assert [a.tolist() for a in t["node_ids"]] == [[0], [1, 2], [3, 4, 9, 10], [5, 6, 7, 8, 11, 12, 13, 14]]
    assert t["routes"][0].tolist() == [[7, 4, 1, 0]] * 4 and t["lrs"][0].tolist() == [[1, 1, -1, 1]] * 4
    assert t["routes"][1].tolist() == [[12, 9, 2, 0]] * 4 and t["lrs"][1].tolist() == [[1, -1, 1, -1]] * 4
    assert t["routes"][2].tolist() == [[7, 4, 1, 0], [5, 3, 1, 0], [8, 4, 1, 0], [6, 3, 1, 0]]
    assert t["lrs"][2].tolist() == [[1, 1, -1, 1], [1, 1, 1, 1], [1, -1, -1, 1], [1, -1, 1, 1]]
    np.testing.assert_allclose(t["probs"][:3], [[1, 0, 0, 0], [1, 0, 0, 0], [0.25, 0.25, 0.25, 0.25]], atol=1e-6)
    assert t["routes"][3].tolist() == t["routes"][0].tolist() and t["lrs"][3].tolist() == t["lrs"][0].tolist() and not t["probs"][3].any()
    with pytest.raises(ValueError):
        D.poi2vec_region_tree(np.array([[0.0, 0.0], [0.0, 1.0]]), 0.2)


def test_loader_on_the_small_file():
    import pandas as pd
    ds, alias = D.load_poi2vec_sequence_file(SMALL, return_aliases=True)
    tab = pd.read_csv(SMALL, sep=" ")
    seqs = [str(s).split("/") for s in tab["u_pois"]]
    times = [[int(v) for v in str(s).split("/")] for s in tab["u_times"]]
    assert ds.n_user == len(seqs) and ds.n_item == len({x for s in seqs for x in s}) == len(alias)
    # split lengths (Load_Data_Poi2vec.py:56, 71-74) and contexts against a brute-force restatement
    for u, (s, t) in enumerate(zip(seqs, times)):
        le = len(s)
        s1, s2 = int(le * 1.0 - 1), int(le * 1.0)
        assert ds.off[u + 1] - ds.off[u] == s1 and ds.tes_off[u + 1] - ds.tes_off[u] == s2 - s1 == 1
        assert [alias[x] for x in s[:s1]] == ds.tra_t[ds.off[u]:ds.off[u + 1]].tolist()
        assert alias[s[s1]] == ds.tes_t[ds.tes_off[u]]
        for j in range(le):
            want = []
            for k in range(j - 1, -1, -1):
                if not t[j] - t[k] < 360:
                    break
                want.append(alias[s[k]])
            if j < s1:
                x = ds.off[u] + j
                got = ds.tra_c[ds.tra_coff[x]:ds.tra_coff[x + 1]]
            else:
                x = ds.tes_off[u]
                got = ds.tes_c[ds.tes_coff[x]:ds.tes_coff[x + 1]]
            assert sorted(got.tolist()) == sorted(want)
    # the tree
    dep = ds.depth
    n_leaf = 1 << (dep - 1)
    assert ds.n_node == 2 * n_leaf - 1 and ds.routes.shape == (ds.n_item + 1, 4, dep) == ds.lrs.shape
    assert np.all(ds.routes[:, :, -1] == 0) and np.all(ds.lrs[:, :, 0] == 1) and np.all(np.abs(ds.lrs) == 1)
    t = D.poi2vec_region_tree(ds.coords, 0.1)
    leaves = set(t["node_ids"][-1].tolist())
    assert len(leaves) == n_leaf and set(ds.routes[:, :, 0].reshape(-1).tolist()) <= leaves
    inner = set(np.concatenate(t["node_ids"][:-1]).tolist()) if dep > 1 else set()
    assert not (set(ds.routes[:, :, 1:].reshape(-1).tolist()) - inner)
    assert sorted(np.concatenate(t["node_ids"]).tolist()) == list(range(ds.n_node))
    assert np.all(ds.probs >= 0) and np.allclose(ds.probs[:-1].sum(axis=1), 1.0, atol=1e-6)
    box = t["leaf_box"][ds.rid[:-1, 0]]
    lat, lon = ds.coords[:, 0], ds.coords[:, 1]
    inside = (lat - 0.05 > box[:, 0]) & (lat + 0.05 < box[:, 1]) & (lon + 0.05 < box[:, 2]) & (lon - 0.05 > box[:, 3])
    assert inside.any()
    np.testing.assert_array_equal(ds.probs[:-1][inside], np.tile(np.float32([1, 0, 0, 0]), (int(inside.sum()), 1)))
    assert np.array_equal(ds.routes[-1], ds.routes[0]) and np.array_equal(ds.lrs[-1], ds.lrs[0]) and not ds.probs[-1].any()
    # a split of (0.6, 0.8): train [0 : int(0.8 le - 1)], test one position
    d2 = D.load_poi2vec_sequence_file(SMALL, split=(0.6, 0.8))
    for u, s in enumerate(seqs):
        assert d2.off[u + 1] - d2.off[u] == int(len(s) * 0.8 - 1) and d2.tes_off[u + 1] - d2.tes_off[u] == int(len(s) * 0.8) - int(len(s) * 0.8 - 1)
    assert d2.n_item == ds.n_item


def test_synthetic_builder():
    ds = D.make_poi2vec_synthetic(30, 120, 14, 3, local=0.5)
    assert ds.n_user == 30 and ds.tra_coff[-1] == len(ds.tra_c) and ds.off[-1] == len(ds.tra_t) == len(ds.tra_coff) - 1
    assert np.all(np.diff(ds.tes_off) == 1) and ds.n_node == (1 << ds.depth) - 1


@pytest.mark.parametrize("softmax_axis", ["reference", "items"])
def test_factorised_scores_equal_the_literal_form(softmax_axis):
    rng = np.random.default_rng(23)
    n_item, dim = 40, 8
    T = _tree(rng, n_item)
    P = _tables(rng, 6, n_item, T["n_node"], dim)
    users = np.array([4, 0, 5])
    cl = rng.uniform(-1.5, 1.5, (3, 2, dim))
    cl[1, 1] = 0.0                                           # an empty context: every indicator 0, paths = 1
    a = O.scores_literal(P, T, users, cl, softmax_axis)
    b = O.scores_factorised(P, T, users, cl, softmax_axis)
    assert a.shape == b.shape == (6, n_item)
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-15)
    plu = O.plu_matrix(P, users, softmax_axis)
    np.testing.assert_allclose(plu.sum(axis=0 if softmax_axis == "reference" else 1), 1.0, rtol=1e-12)
    np.testing.assert_allclose(a[3], plu[1], rtol=1e-12)     # row (user 1, position 1): paths = 1
    assert np.array_equal(O.topk_desc(np.array([[1.0, 3.0, 3.0, 2.0]]), 3), [[1, 2, 3]])


def test_poi2vec_declarations_match_signatures():
    hdr = open(os.path.join(ROOT, "include", "poi_hip.h")).read()
    assert poi_amd._lib.ABI_VERSION == 9 and "#define POI_ABI_VERSION 9" in hdr
    for name, nargs in (("poi_poi2vec_step", 15), ("poi_poi2vec_scores", 11), ("poi_poi2vec_topk", 13)):
        m = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(poi_amd._lib.SIGNATURES[name][1]), name
    i = hdr.index("---- POI2Vec (additive to ABI 9)")
    assert hdr.index("---- GeoIE (additive to ABI 9)") < i < hdr.index("---- multi-GPU")
    block = hdr[i:hdr.index("---- multi-GPU", i)]
    for s in ("POI2Vec.py", "Load_Data_Poi2vec.py", "len_max", '"p2v_dense"', '"p2v_pos"', '"p2v_sc_node"', '"p2v_sc_topk"'):
        assert s in block, s
    m = re.search(r"typedef struct poi_poi2vec_params \{(.*?)\} poi_poi2vec_params;", hdr, re.S)
    fields = [f.strip().split()[-1].lstrip("*") for f in m.group(1).split(";") if f.strip()]
    assert fields == [f[0] for f in poi_amd._lib.Poi2vecParams._fields_]
