"""The catalogue of chosen PFOR128 group shapes (tests/pfor_cases.py) is what it claims — on the CPU, from the host encoder's BYTES, because nothing on the device
reports which decoder path a row took.

  * every shape list's groups carry the intended header word (b, nexc, eb) and the intended exception count per quarter, and the other side of the block is plain;
  * TABLE (shape -> list) names what every list is there for; each entry is recomputed from the parsed headers, the table's lists are exactly the catalogue (a list
    removed from either fails), and REQUIRED — every deltas width 1 .. 20, every freqs width 0 .. 16, every per-quarter count, both sides of the fast / fallback
    boundary, both arms of the joint rule, every refill count — is reached;
  * the literals the table restates (k_fused.hpp: the fallback predicate `cnt > 16 || cnt * eb > 64`, the refill rule `b > NW`, NW = 8 for deltas and 4 for freqs)
    are parsed out of the header, so the table fails when the kernel's constants move;
  * under the default options no shape list has a term plane (with plane_div = 64 no catalogue list has), the dense partner has one, and every `L OR p_dense` and
    `p_dense OR union` plans as a k_psets scatter union: the one place where k_psets' scatter (PscatPost, a user of PfRegs<8>) decodes the catalogue;
  * from the bytes alone: HostIndex (the upload walk, h_ints_decode) accepts both corpora, the oracle decodes them back to the input, and
    oracle/trinity_oracle_lucene.c writes the same bytes as host/lucene_encoder.hpp.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import pfor_cases as PC
import structured as S
import trinity_amd as T
from test_structured import kinds_of_queries
from trinity_amd import hostplan as HP

WHICH = ["narrow", "wide"]


@pytest.fixture(scope="module")
def corpora():
    T.build.build_host()
    O.lib()
    return {w: PC.corpus(w) for w in WHICH}


# ---- the kernel's literals ------------------------------------------------------------------------------------------------------------------------
def test_kernel_literals_mirror():
    """k_fused.hpp, PfRegs::init: `if (cnt > 16 || cnt * eb > 64) return false;`; PfRegs::next: `r && used == NW / 2 && b > NW`; row_decode: `PfRegs<8> rd;` reads
    the deltas group (header rec_z), `PfRegs<4> rf;` the freqs group behind it (header rec_w), and the rows go to row_streams_lucene unless `okd && okf`."""
    text = re.sub(r"//[^\n]*", "", open(os.path.join(S.CSRC, "k_fused.hpp")).read())
    m = re.search(r"if\s*\(cnt > (\d+) \|\| cnt \* eb > (\d+)\)\s*return false;", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (PC.FAST_MAX_CNT, PC.FAST_MAX_BITS)
    assert re.search(r"const bool f = r && used == NW / 2 && b > NW;", text)
    rd, rf = re.search(r"PfRegs<(\d+)> rd;", text), re.search(r"PfRegs<(\d+)> rf;", text)
    assert (int(rd.group(1)), int(rf.group(1))) == (PC.NW_DELTAS, PC.NW_FREQS)
    assert re.search(r"okd = rd\.init\(g, rec_z,", text) and re.search(r"rf\.init\(g \+ pfor_group_bytes\(rec_z\), rec_w,", text) and re.search(r"if \(okd && okf\)", text)
    assert [PC.refills(b, 8) for b in (8, 9, 12, 13, 16, 17, 20)] == [0, 1, 1, 2, 2, 3, 3] and [PC.refills(b, 4) for b in (4, 5, 6, 7, 16)] == [0, 1, 1, 2, 6]
    assert not PC.falls_back(16, 4) and not PC.falls_back(4, 16) and PC.falls_back(13, 5) and PC.falls_back(4, 17) and PC.falls_back(17, 1)
    k = S.header_constants("dev_structs.hpp", "pfor128_group.hpp", "lucene_enc_units.hpp")
    assert k["LENC_BLOCK"] == PC.BLOCK


# ---- every list has its shape -----------------------------------------------------------------------------------------------------------------------
def side_headers(c, name):
    side = PC.SHAPES[name][0]
    t = c.tid[name]
    return PC.hits_headers(c, t) if side == "h" else [h[0 if side == "d" else 1] for h in PC.index_headers(c, t)]


@pytest.mark.parametrize("which", WHICH)
def test_every_shape_list_has_the_intended_headers(corpora, which):
    c = corpora[which]
    for name, (side, corpus, b, counts, eb, groups) in PC.SHAPES.items():
        if corpus != which:
            continue
        hs = side_headers(c, name)
        assert len(hs) == groups, (name, len(hs))
        for h in hs:
            if isinstance(b, tuple):
                assert h == b, (name, h)
            else:
                assert h[:3] == (b, sum(counts), eb) and tuple(h[3]) == counts, (name, h[:4], (b, sum(counts), eb, counts))
        if side != "h":  # the other side of the block is plain: no exceptions there
            for pair in PC.index_headers(c, c.tid[name]):
                other = pair[1 if side == "d" else 0]
                assert other[0] != "eq" and other[1] == 0, (name, other)
            d, f = c.lists[name]
            assert d.size == groups * PC.BLOCK + len(PC.TAIL_DELTAS)  # whole blocks, then a varbyte tail
    if which == "narrow":
        assert int(c.freqs.max()) == (1 << PC.FREQ_BITS) - 1  # the write side admits every 16-bit frequency: the freqs widths go to 16
        f0 = c.lists["f_x_w0_e1"][1]
        assert int((f0 == 0).sum()) > 200 and int((f0 > 0).sum()) >= 6


# ---- the coverage table -------------------------------------------------------------------------------------------------------------------------
def vbytes(v):
    return 1 if v < 1 << 7 else 2 if v < 1 << 14 else 3 if v < 1 << 21 else 4 if v < 1 << 28 else 5


def reach(side, headers, nw):
    """What a list's groups of one side reach, from their parsed headers."""
    out = set()
    for h in headers:
        if h[0] == "eq":
            out.add(f"{side}:eq{vbytes(h[1])}")
            continue
        b, nexc, eb, cnt, e0, epos = h
        out.add(f"{side}:w{b}")
        if nw:
            out.add(f"{side}:refill{PC.refills(b, nw)}")
        if not nexc:
            out.add(f"{side}:plain{b}")
            continue
        out.add(f"{side}:eb{eb}")
        have = [q for q in range(4) if cnt[q]]
        if any(not cnt[q] for q in range(have[0], have[-1])):
            out.add(f"{side}:gap")
        if have == [3]:
            out.add(f"{side}:q3only")
        for q in have:
            out.add(f"{side}:cnt{cnt[q]}")
            out.add(f"{side}:{'slow' if PC.falls_back(cnt[q], eb) else 'fast'}{cnt[q]}x{eb}")
            if e0[q]:
                out.add(f"{side}:hs0" if e0[q] * eb % 8 == 0 else f"{side}:hs+")
        out |= {f"{side}:pos{p % 32}" for p in epos if p % 32 in (0, 31)}
    if len({h[:3] for h in headers}) >= 10:
        out.add(f"{side}:mixed")
    return out


def reach_list(c, name):
    """Everything list `name` reaches: both sides of its blocks, the joint rule row by row, its hits.data groups."""
    t = c.tid[name]
    pairs = PC.index_headers(c, t)
    out = reach("d", [p[0] for p in pairs], PC.NW_DELTAS) | reach("f", [p[1] for p in pairs], PC.NW_FREQS)
    for hd, hf in pairs:
        for q in range(4):
            cd, cf = (0 if hd[0] == "eq" else hd[3][q]), (0 if hf[0] == "eq" else hf[3][q])
            sd, sf = cd and PC.falls_back(cd, hd[2]), cf and PC.falls_back(cf, hf[2])
            out |= {"joint:d_slow_f_fast"} if sd and not sf else {"joint:f_slow_d_fast"} if sf and not sd else {"joint:both_x_fast"} if cd and cf and not sd and not sf else set()
    hh = PC.hits_headers(c, t)
    out |= reach("h", hh, 0)
    f = c.lists[name][1].astype(np.int64)
    ends = np.cumsum(f)
    for e, k in zip(ends.tolist(), f.tolist()):  # a document whose hits lie in two groups of different headers
        g0, g1 = (e - k) // PC.BLOCK, (e - 1) // PC.BLOCK
        if k > 1 and g0 != g1 and g1 < len(hh) and hh[g0][:3] != hh[g1][:3]:
            out.add("h:straddle")
    return out


# shape -> list: what every list of the catalogue is there for (its plain side and whatever else its groups happen to reach are not listed)
TABLE = {
    **{f"d_w{w}": {f"d:plain{w}", f"d:refill{PC.refills(w, 8)}"} for w in range(2, 21)},
    "d_eq1": {"d:eq1"}, "d_eq2": {"d:eq2"}, "d_eq3": {"d:eq3"},
    "d_x_1_8_0_9": {"d:cnt1", "d:cnt8", "d:cnt9", "d:gap", "d:eb4", "d:hs+", "d:pos0", "d:pos31", "d:fast9x4"},
    "d_x_2_16": {"d:cnt16", "d:fast16x4", "d:hs0"},
    "d_x_4x16": {"d:w1", "d:eb16", "d:fast4x16", "d:hs0"},
    "d_x_13x5": {"d:eb5", "d:slow13x5", "d:fast1x5", "joint:d_slow_f_fast"},
    "d_x_4x17": {"d:w1", "d:eb17", "d:slow4x17", "d:fast1x17", "joint:d_slow_f_fast"},
    "d_x_17": {"d:cnt17", "d:slow17x2", "joint:d_slow_f_fast"},
    "d_x_32": {"d:cnt32", "d:slow32x4", "joint:d_slow_f_fast"},
    "d_x_q3": {"d:q3only", "d:eb1", "d:pos0", "d:pos31"},
    "d_x_e5": {"d:eb5", "d:hs+", "d:pos0", "d:pos31"},
    "d_x_e8": {"d:eb8", "d:hs0"},
    "d_x_ebmax": {"d:w1", "d:eb25", "d:pos31"},
    **{f"f_w{w}": {f"f:plain{w}", f"f:refill{PC.refills(w, 4)}"} for w in range(1, 17)},
    "f_eq0": {"f:eq1"}, "f_eq1": {"f:eq1"}, "f_eq2": {"f:eq2"},
    "f_x_1_8_0_9": {"f:cnt1", "f:cnt8", "f:cnt9", "f:gap", "f:eb4", "f:hs+", "f:pos0", "f:pos31"},
    "f_x_2_16": {"f:cnt16", "f:fast16x4", "f:hs0"},
    "f_x_4x16": {"f:w0", "f:eb16", "f:fast4x16", "f:hs0"},
    "f_x_13x5": {"f:eb5", "f:slow13x5", "joint:f_slow_d_fast"},
    "f_x_17": {"f:cnt17", "f:slow17x2", "joint:f_slow_d_fast"},
    "f_x_32": {"f:cnt32", "f:slow32x4", "joint:f_slow_d_fast"},
    "f_x_q3": {"f:q3only", "f:eb1", "f:pos0", "f:pos31"},
    "f_x_e5": {"f:eb5", "f:hs+"},
    "f_x_e8": {"f:eb8", "f:hs0"},
    "f_x_w0_e1": {"f:w0", "f:eb1"},
    "f_x_w0_e9": {"f:w0", "f:eb9", "f:pos0", "f:pos31"},
    "x_both": {"joint:both_x_fast"},
    "mixed_d": {"d:mixed"},
    "mixed_f": {"f:mixed"},
    **{f"h_w{w}": {f"h:plain{w}"} for w in range(1, 15)},
    "h_eq": {"h:eq1"}, "h_x1": {"h:cnt1"}, "h_x9": {"h:cnt9"}, "h_x17": {"h:cnt17"}, "h_straddle": {"h:straddle"},
}  # fmt: skip
# the union the catalogue must reach.  Not admitted by the value ranges (pfor_cases.py): d:plain1 / h has it only through repeated positions; f:slow4x17 (b + eb <= 16);
# deltas widths 21 .. 32 and eb > 25 (D <= 2^26 + 37)
REQUIRED = (
    [f"d:w{w}" for w in range(1, 21)] + [f"d:plain{w}" for w in range(2, 21)] + ["d:eq1", "d:eq2", "d:eq3"] + [f"d:refill{r}" for r in range(4)]
    + [f"f:w{w}" for w in range(0, 17)] + [f"f:plain{w}" for w in range(1, 17)] + ["f:eq1", "f:eq2"] + [f"f:refill{r}" for r in range(7)]
    + [f"{s}:cnt{n}" for s in "df" for n in (1, 8, 9, 16, 17, 32)] + [f"{s}:{x}" for s in "df" for x in ("gap", "q3only", "pos0", "pos31", "hs0", "hs+", "mixed")]
    + [f"d:eb{e}" for e in (1, 4, 5, 8, 16, 17, 25)] + [f"f:eb{e}" for e in (1, 4, 5, 8, 9, 16)]
    + ["d:fast16x4", "d:fast4x16", "d:slow13x5", "d:slow4x17", "f:fast16x4", "f:fast4x16", "f:slow13x5"]
    + ["joint:d_slow_f_fast", "joint:f_slow_d_fast", "joint:both_x_fast"]
    + [f"h:plain{w}" for w in range(1, 15)] + ["h:eq1", "h:cnt1", "h:cnt9", "h:cnt17", "h:straddle"]
)  # fmt: skip


def test_the_table_is_the_catalogue_and_reaches_every_shape(corpora):
    lists = {n: w for w in WHICH for n in PC.catalogue(w) if n != "mixed_d"}
    assert sorted(set(lists) | {"mixed_d"}) == sorted(TABLE), sorted((set(lists) | {"mixed_d"}) ^ set(TABLE))
    reached = set()
    for name, want in TABLE.items():
        for which in WHICH if name == "mixed_d" else [lists[name]]:
            assert name in corpora[which].tid, (which, name)
            got = reach_list(corpora[which], name)
            assert want <= got, (which, name, sorted(want - got))
            reached |= want if name.startswith("mixed") else got  # (a shape counts in its own list, not where a mixed list repeats it)
    assert set(REQUIRED) <= reached, sorted(set(REQUIRED) - reached)
    for which in WHICH:  # the mixed lists hold every shape of their side and corpus, one block each
        c = corpora[which]
        for side, mixed in (("d", "mixed_d"), ("f", "mixed_f")):
            shapes = [n for n, s in PC.SHAPES.items() if s[0] == side and s[1] == which]
            if not shapes:
                continue
            pairs = PC.index_headers(c, c.tid[mixed])
            got = sorted(str(p[side == "f"][:4]) for p in pairs)
            assert got == sorted(str(side_headers(c, n)[0][:4]) for n in shapes), (which, mixed)
            assert len(pairs) >= 12  # a wave's 64 lanes take the rows of 16 consecutive groups: differently shaped ones at once


# ---- where k_psets' scatter decodes the catalogue -------------------------------------------------------------------------------------------------------
PSET_UNIT_SCATTER = 4  # csrc/dev_structs.hpp (DevPsetUnit::first)


@pytest.mark.parametrize("which", WHICH)
def test_unions_with_the_dense_partner_are_scatter_unions(corpora, which):
    """The planner gives a term a plane from df >= docs / plane_div on (default 1024) and runs a DocumentsOnly union of plane terms with plane-less ones in k_psets,
    listing the plane-less terms' documents through row_decode (PSET_UNIT_SCATTER).  Default options: every shape list, x_both and the hits lists are plane-less
    (the narrow corpus' mixed lists, 3 .. 4 K documents, are not); plane_div = 64 on the narrow corpus: every catalogue list is."""
    k = S.header_constants("dev_structs.hpp")
    assert k["PSET_UNIT_SCATTER"] == PSET_UNIT_SCATTER
    c = corpora[which]
    cat = PC.catalogue(which)
    plain = [n for n in cat if which == "wide" or not n.startswith("mixed")]
    hi = c.host_index(2)
    try:
        for opts, names in (({}, plain), (PC.SCATTER_OPTS, cat)) if which == "narrow" else (({}, cat),):
            texts = [f"{{{n}}} OR {{p_dense}}" for n in names] + (PC.union_queries(which) if names == cat else [])
            queries = [(c.q(t), 1) for t in texts]
            p = HP.HostPlan(hi, S.programs(queries), T.FLAG_DOCUMENTS_ONLY, 0, threads=2, options=opts)
            try:
                planes = {c.names[t] for t in p.plane_terms.tolist()}
                assert "p_dense" in planes and not planes & set(names), (opts, sorted(planes & set(names)))
                assert p.s["unsupported_queries"] == 0 and (kinds_of_queries(p, len(queries)) == HP.TASK_PSET).all(), opts
                u = p.units  # every unit of the batch is a scatter unit, and every query owns some
                assert ((u["first"] & PSET_UNIT_SCATTER) != 0).all() and np.unique(p.tasks["slot"][u["tix"]]).size == len(queries), (opts, u.size, len(queries))
            finally:
                p.close()
    finally:
        hi.close()


# ---- from the bytes alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH)
def test_the_upload_walk_accepts_the_corpus(corpora, which):
    from trinity_amd import hostplan as HP

    c = corpora[which]
    hi = c.host_index(2)  # (raises TrinityError on a group the walk does not take)
    try:
        assert isinstance(hi, HP.HostIndex)
        for t in range(len(c.names)):  # ... and it finds the whole 128-hit groups the parse above finds
            assert hi.hits_dir(t)[1] == len(PC.hits_headers(c, t)), c.names[t]
    finally:
        hi.close()


def oracle_lucene(c):
    """The oracle's own Lucene-shaped encoding of the corpus' postings (oracle/trinity_oracle_lucene.c: a frequency-0 document is a token at position 0)."""
    f = c.freqs.astype(np.int64)
    reps = np.maximum(f, 1)
    tok_doc = np.repeat(c.docs, reps).astype(np.uint32)
    tok_pos = np.zeros(tok_doc.size, dtype=np.uint16)
    tok_pos[np.repeat(f > 0, reps)] = c.pos
    ends = np.concatenate([[0], np.cumsum(reps)])
    term_off = ends[c.term_first.astype(np.int64)].astype(np.uint64)
    corpus = O.ToCorpus(c.docs_cnt, len(c.names), 0, tok_doc.size, term_off.ctypes.data_as(C.POINTER(C.c_uint64)), tok_doc.ctypes.data_as(C.POINTER(C.c_uint32)),
                        tok_pos.ctypes.data_as(C.POINTER(C.c_uint16)))  # fmt: skip
    return O.Index(O.lib().to_lucene_encode(C.byref(corpus)))


@pytest.mark.parametrize("which", WHICH)
def test_both_encoders_write_the_same_bytes_and_the_oracle_reads_them_back(corpora, which):
    c = corpora[which]
    ix = oracle_lucene(c)
    assert np.array_equal(ix.terms(), c.l_terms)
    assert np.array_equal(ix.bytes(), c.l_index) and np.array_equal(ix.hits(), c.l_hits)
    for t, n in enumerate(c.names):
        d, f = ix.decode_term(t)
        assert np.array_equal(d, c.lists[n][0]) and np.array_equal(f, c.lists[n][1]), n
    for n in [x for x in c.names if x.startswith("h_") or x.startswith("n_h_")]:  # positions, document by document, of the lists with written positions
        it, got = O.PLI(ix, c.tid[n]), []
        while it.next() != O.DOCIDS_END:
            got += it.positions()
        assert got == c.positions[n].tolist(), n
