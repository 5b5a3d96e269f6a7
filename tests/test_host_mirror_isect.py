"""Trinity::intersect on the C++ operator surface (trinity_amd/csrc/host/trinity_gpu.hpp: intersect_impl / intersect over one source with a registry, intersect over an
IndexSourcesCollection, intersection_indices, sort_intersections).  The driver tests/cpp/host_mirror_isect_test.cpp runs the requests over two segments — the newer
one updates documents of the older, so the older runs under a registry — and prints every list; they must equal the restatement of tests/isect_cases.py per source,
and its lists sorted by mask with equal masks summed (intersect.cpp:184-199) for the collection."""
import os
import subprocess

import numpy as np
import pytest

import isect_cases as IC
import structured as S

TOP = 70000


def sources():
    """Two sources over tokens a, b, c1 / c2 (synonyms) and x.  Source 0 (older): the gadget of isect_cases with a document the newer source updates and an origMask
    document inside the run.  Source 1 does not know c2 (origMask = 0 there: a document that holds every group is counted); both sources hold {a}-only and {a, b} documents — masks of both."""
    at = 5 * IC.SPAN - 4
    ev0 = IC.gadget(at, [at + i for i in (1, 2, 4, 6, 7, 8)], [(at + 3, ["b"]), (at + 5, ["a", "b", "c1"])]) + [(9, ["a", "c2"]), (10, ["a", "c1", "c2"]), (11, ["a", "c2"]), (40000, ["x"])]
    ev1 = [(3, ["a", "b"]), (4, ["a"]), (5, ["a"]), (6, ["a", "b", "c1"]), (7, ["a", "b", "c1"]), (8, ["b"]), (60000, ["a", "b"]), (60001, ["x", "b"])]
    names = [["a", "b", "c1", "c2", "x"], ["a", "b", "c1", "x"]]
    out = []
    for ev, nm in zip((ev0, ev1), names):
        lists = {n: [] for n in nm}
        for d, ts in ev:
            for t in ts:
                lists[t].append(d)
        out.append({n: np.unique(np.asarray(v, dtype=np.int64)) for n, v in lists.items()})
    updates = [[], [at + 3, 40000]]  # source 1 re-indexes two documents of source 0
    return out, updates


REQUESTS = [(0, [["a"], ["b"], ["c1", "c2"]]), (1 << 2, [["a"], ["b"], ["c1", "c2"]]), (0, [["x"], ["a"]]), (0, [["nosuch"], ["c2"]]), (0, [["b"], ["a"], ["x", "nosuch"]])]


def expected(srcs, updates):
    per, coll = [], []
    for stop, groups in REQUESTS:
        lists = []
        for s, L in enumerate(srcs):
            masked = sorted({d for u in updates[s + 1 :] for d in u})
            g = [[L.get(t, IC.UNKNOWN) for t in grp] for grp in groups]
            lists.append(IC.restate(g, stop, masked, top=TOP)[0])
        per.append(lists)
        acc = {}
        for l in lists:
            for m, n in l:
                acc[m] = (acc.get(m, 0) + n) & 0xFFFFFFFF
        coll.append(sorted(acc.items()))
    return per, coll


def test_the_expected_lists_cover_what_the_test_is_about():
    srcs, updates = sources()
    per, coll = expected(srcs, updates)
    assert 2 in dict(per[2][0]) and 2 in dict(per[2][1])  # request 2: {a} in both sources ...
    assert dict(coll[2])[2] == dict(per[2][0])[2] + dict(per[2][1])[2] and len(coll[2]) == 2  # ... summed; {x} from one source only
    assert 7 in dict(per[0][1]) and 7 not in dict(per[0][0])  # origMask is per source: source 1 does not know c2, so {a, b, c} counts there
    no_registry = IC.restate([[srcs[0][t] for t in g] for g in REQUESTS[0][1]], 0, (), top=TOP)[0]
    assert no_registry != per[0][0]  # the registry matters
    assert per[3] == [[(2, 3)], []] and per[1][0] != per[0][0]  # a source that knows one token only; the stop word changes the answer


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


def test_isect_mirror_compiles_and_links(T):
    from trinity_amd.build import MIRROR_ISECT_BIN

    assert os.path.exists(MIRROR_ISECT_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_ISECT_BIN], capture_output=True, text=True).stdout


@pytest.mark.gpu
def test_single_source_and_collection_equal_the_restatement(T, tmp_path):
    from trinity_amd.build import MIRROR_ISECT_BIN

    srcs, updates = sources()
    rpath = str(tmp_path / "requests")
    with open(rpath, "w") as f:
        for stop, groups in REQUESTS:
            f.write(" ".join([str(stop), str(len(groups))] + [" ".join([str(len(g))] + g) for g in groups]) + "\n")
    args = [MIRROR_ISECT_BIN, rpath]
    for s, L in enumerate(srcs):
        c = S.build({n: (d.astype(np.uint32), np.ones(d.size, dtype=np.uint32)) for n, d in L.items()}, docs_cnt=TOP)
        ipath, tpath, npath, upath = (str(tmp_path / f"{k}{s}") for k in ("index", "terms", "names", "updates"))
        np.asarray(c.g_index).tofile(ipath)
        np.ascontiguousarray(c.g_terms, dtype=np.uint32).tofile(tpath)
        open(npath, "w").write("".join(n + "\n" for n in c.names))
        np.asarray(updates[s], dtype=np.uint32).tofile(upath)
        args += [ipath, tpath, npath, str(TOP), upath]
    res = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    single, coll, indices = {}, {}, {}
    for l in res.stdout.splitlines():
        w = l.split()
        pairs = lambda ws: [tuple(int(x) for x in p.split(":")) for p in ws]
        if w[0] == "single":
            assert int(w[3]) == len(w) - 4
            single[(int(w[1]), int(w[2]))] = pairs(w[4:])
        elif w[0] == "collection":
            assert int(w[2]) == len(w) - 3
            coll[int(w[1])] = pairs(w[3:])
        elif w[0] == "indices":
            indices[int(w[1])] = [int(x) for x in w[2:]]
    assert "refused 2" in res.stdout.splitlines()
    per, cwant = expected(srcs, updates)
    for r in range(len(REQUESTS)):
        for s in range(2):
            assert single[(r, s)] == per[r][s], (r, s)
        assert coll[r] == cwant[r], r
        if cwant[r]:
            best = max(cwant[r], key=lambda e: (bin(e[0]).count("1"), e[1]))  # sort_intersections: popcount, then count
            top = [e for e in cwant[r] if (bin(e[0]).count("1"), e[1]) == (bin(best[0]).count("1"), best[1])]
            assert indices[r] in [[i for i in range(64) if m >> i & 1] for m, _ in top], r
