"""The wide tree kernels at the record's limits and the chunk edges (a helper module, imported by tests/test_wide_tree_cases.py, tests/test_gpu_wide_tree_limits.py
and tests/test_gpu_perc.py): one structured corpus, a catalogue of named trees, a replay of csrc/tree_fold.hpp in Python integers and a restatement of which
leaves k_tree_leaves_wide scores.

The corpus `wtree` (structured.build): D = 4 C + 37 with C = 32 TREE_CHUNK_WORDS, the documents one workgroup of k_tree_eval_wide folds — the documents reach two bitmap
words into a fifth chunk (the planner rounds a row up to whole SPAN_BITS windows: plw = 16 384 words, eight chunks, of which 2 and 5 .. 7 hold nothing and 4 holds two words'
worth).  Only the ACTIVE documents hold anything: [1, 4096] (chunk 0 is busy), [C - 64, C + 64] (chunk 1 holds its first 65 documents only), nothing in chunk 2,
[3C, 3C + 64] and [4C - 64, D] (chunk 3: a head and a tail; chunk 4: the short last chunk, D its last bit).
  * ladder lists L0 .. L59: Li holds the active document d iff i < d % 61, so d is held by exactly h(d) = d % 61 of them — every count 0 .. 60 occurs and a matchsome
    over ladder leaves has a closed form; frequencies LADDER_FREQS by (rank + i) (both sides of PL_NESTED, and f = 0: k_tree_leaves_wide's lookup);
  * partition lists P0 .. P63: Pi holds the active d iff d % 64 == i (disjoint; their union is every active document); frequencies 1 .. 3 by rank.
Term ids: L0 .. L59 are 0 .. 59 — the same programs are stored queries of a percolator over 60 terms (perc_programs / perc_docs) —, P0 .. P63 are 60 .. 123.

Ladder sets are nested, so every tree over ladder leaves answers "h(d) >= t" for some t: CLOSED gives t where it has been worked out by hand."""
import numpy as np

import oracle_lib as O
import structured as S

C = S.TREE_CHUNK_WORDS * 32
D = 4 * C + 37
NLADDER, NPART, HMOD = 60, 64, 61
LADDER_FREQS = [0, 1, 2, 3, 4, 5, 6, 7, 16]
WIDE = {"tree_max_nodes": 1024}
STACK_REASON = "more than 64 words of evaluation stack"
MUTANTS = ("thr_byte", "planes8", "stack32", "nodes64")
OP_TERM, OP_AND, OP_OR, OP_NOT, OP_OPT, OP_SOME = O.OP_TERM, O.OP_AND, O.OP_OR, O.OP_NOT, O.OP_OPT, O.OP_SOME


def active_docs():
    ar = np.arange
    return np.concatenate([ar(1, 4097), ar(C - 64, C + 65), ar(3 * C, 3 * C + 65), ar(4 * C - 64, D + 1)]).astype(np.int64)


def corpus():
    act = active_docs()
    lists = {}
    for i in range(NLADDER):
        d = act[act % HMOD > i]
        lists[f"L{i}"] = (d.astype(np.uint32), np.array(LADDER_FREQS, dtype=np.int64)[(np.arange(d.size) + i) % len(LADDER_FREQS)])
    for i in range(NPART):
        d = act[act % NPART == i]
        lists[f"P{i}"] = (d.astype(np.uint32), 1 + np.arange(d.size) % 3)
    c = S.build(lists)
    assert c.D == D and [c.tid[f"L{i}"] for i in range(NLADDER)] == list(range(NLADDER))
    return c


def h_of(docs):
    return np.asarray(docs, dtype=np.int64) % HMOD


# ---- the programs (postfix, oracle_lib.tok) ---------------------------------------------------------------------------------------------------
def tk(*terms):
    return [O.tok(OP_TERM, int(t)) for t in terms]


def ladder(n, first=0, mod=NLADDER):
    """n leaves L((first + i) % mod)"""
    return tk(*[(first + i) % mod for i in range(n)])


def flat(op, n, **kw):
    return ladder(n, **kw) + [O.tok(op, n)]


def some(n, thr):
    return ladder(n) + [O.tok(OP_SOME, (thr << 16) | n)]


def deep(levels, leaf_of):
    """Right-deep alternation AND(t0, OR(t1, AND(t2, ...))): level k is AND (k even) or OR over the leaf leaf_of(k) and, as its LAST child, level k + 1 — the innermost
    level's last child is the leaf leaf_of(levels).  Every level's accumulator is open at that leaf: `levels` stack words."""
    return tk(*[leaf_of(k) for k in range(levels + 1)]) + [O.tok(OP_OR if k % 2 else OP_AND, 2) for k in range(levels - 1, -1, -1)]


def chain(level_leaf, some_leaves):
    """Eight alternating AND / OR levels (as deep()), then eight nested matchsomes of 100 children and minimum 2, each inner one the LAST child of the one around it:
    8 + 8 x 7 stack words at the innermost matchsome's leaves.  level_leaf(k): level k's leaf; some_leaves(j, n): the n leaf terms of matchsome j (7: the innermost)."""
    prog = tk(*[level_leaf(k) for k in range(8)])
    for j in range(8):
        prog += tk(*some_leaves(j, 100 if j == 7 else 99))
    prog += [O.tok(OP_SOME, (2 << 16) | 100)] * 8
    return prog + [O.tok(OP_OR if k % 2 else OP_AND, 2) for k in range(7, -1, -1)]


def _chain_plain():
    at = [8]  # (the running leaf number: the levels' leaves are 0 .. 7)

    def leaves(j, n):
        at[0] += n
        return [(at[0] - n + i) % NLADDER for i in range(n)]

    return chain(lambda k: k, leaves)


def _chain_inner():
    """The innermost matchsome decides: matchsome j holds L(j) once and 98 leaves of L40 .. L59, so for 7 < h <= 40 it counts 1 + the matchsome inside it; the innermost
    holds L7, L25 and 98 of L40 .. L59: h >= 26.  The AND levels' leaves are L6, L4, L2, L0 from the root down (wide, and each cheaper than the level below it: the parser
    sorts an AND's children by cost, and the deep child has to stay the last), the OR levels' L58 .. L52 (narrow): for 6 < h <= 52 the levels hand the chain up."""
    return chain(lambda k: 59 - k if k % 2 else 6 - k, lambda j, n: [j] + ([25] if j == 7 else []) + [40 + i % 20 for i in range(98)])


def _deep_inner(levels=64):
    """AND levels over L0, OR levels over L11, the innermost leaf L5: for h <= 11 every level hands the deepest leaf's value up — h >= 6."""
    return deep(levels, lambda k: 5 if k == levels else 11 if k % 2 else 0)


# name -> (program, header (nnodes, stack words, depth), root (cbits, thr, nkids))
def cases():
    part = tk(*range(NLADDER, NLADDER + NPART)) + [O.tok(OP_OR, NPART)]
    out = {"or1023": (flat(OP_OR, 1023), (1024, 1, 1), (0, 0, 1023))}
    for thr in (255, 256, 260, 300):
        out[f"some300_{thr}"] = (some(300, thr), (301, 9, 1), (9, thr, 300))
    for thr in (1, 510, 511, 1020):
        out[f"some1020_{thr}"] = (some(1020, thr), (1021, 10, 1), (10, thr, 1020))
    out["deep64"] = (deep(64, lambda k: k % 12), (129, 64, 64), (0, 0, 2))
    out["deep64_inner"] = (_deep_inner(), (129, 64, 64), (0, 0, 2))
    out["somechain"] = (_chain_plain(), (817, 64, 16), (0, 0, 2))
    out["somechain_inner"] = (_chain_inner(), (817, 64, 16), (0, 0, 2))
    out["allP"] = (part, (65, 1, 1), (0, 0, NPART))
    out["not_wide"] = (tk(0) + tk(*[1 + i % 59 for i in range(500)]) + [O.tok(OP_OR, 500), O.tok(OP_NOT, 2)], (503, 2, 2), (0, 0, 2))  # h == 1
    # a required term and an optional OR of TERMS is a conjunction with an optional group to the planner — no tree record in any mode (header None): it runs, beside the
    # trees, through the kernels the narrow tests cover; opt_wide_tree's optional side is an OR of 250 conjunctions, which only a tree holds
    out["opt_wide"] = (tk(1) + flat(OP_OR, 500) + [O.tok(OP_OPT, 2)], None, None)
    pairs = sum((tk(i % NLADDER, (i + 7) % NLADDER) + [O.tok(OP_AND, 2)] for i in range(250)), [])
    out["opt_wide_tree"] = (tk(1) + pairs + [O.tok(OP_OR, 250), O.tok(OP_OPT, 2)], (753, 3, 3), (0, 0, 2))
    return {k: (np.array(p, dtype=np.uint32), hdr, root) for k, (p, hdr, root) in out.items()}


def left_out():
    """name -> (program, status, reason): the boundary from the other side."""
    return {"deep65": (np.array(deep(65, lambda k: k % 12), dtype=np.uint32), -3, STACK_REASON)}


NAMES = list(cases())
TREE_NAMES = [n for n, (_, hdr, _) in cases().items() if hdr is not None]
SOME_CASES = {f"some300_{t}": (5, t) for t in (255, 256, 260, 300)} | {f"some1020_{t}": (17, t) for t in (1, 510, 511, 1020)}  # name -> (leaves per ladder list, threshold)
# the least h(d) a case matches, worked out by hand (the matchsomes: ceil(thr / multiplicity))
CLOSED = {n: -(-t // m) for n, (m, t) in SOME_CASES.items()} | {"or1023": 1, "deep64": 2, "deep64_inner": 6, "somechain": 2, "somechain_inner": 26, "opt_wide": 2, "opt_wide_tree": 2}
SCORED_TFIDF = ("or1023", "some1020_511")
RICH_DEFAULT, RICH_WIDE = ("deep64",), ("or1023", "some300_260")  # default rich_max_terms (12 reportable terms) / rich_max_terms = 64 (60 of them)
PERC_CASES = [n for n in NAMES if n.startswith(("some", "or1023", "deep64"))]


def chunk_edge_mask():
    """The masked set of the GPU file: the documents on bits 0 / 31 of the chunks' first / last words, and every seventh active document."""
    return np.unique(np.concatenate([[1, 31, 32, C - 1, C, C + 1, 3 * C, 4 * C - 1, 4 * C, D], active_docs()[::7]])).astype(np.uint32)


def filter_drop():
    """What the TRI_FILTER_DROP filter of the GPU file drops: every fifth active document (from the third), D - 1 and the first document of chunk 1."""
    return np.unique(np.concatenate([active_docs()[2::5], [C, D - 1]])).astype(np.uint32)


# ---- the percolator's view: the ladder as documents ---------------------------------------------------------------------------------------------
PERC_NDOCS = 130


def perc_programs():
    cs = cases()
    return [cs[n][0].tolist() for n in PERC_CASES]


def perc_docs():
    """Document j holds terms 0 .. (j % 61) - 1, each at one position: h(j) = j % 61, as in the corpus."""
    return [{t: [t + 1] for t in range(j % HMOD)} for j in range(PERC_NDOCS)]


# ---- the fold of csrc/tree_fold.hpp over a planner's wide record ------------------------------------------------------------------------------------
def bits_of(docs, act=None):
    """A docID set as a Python integer: bit r = the r-th active document."""
    act = active_docs() if act is None else act
    out = 0
    for r in np.searchsorted(act, np.asarray(docs, dtype=np.int64)).tolist():
        out |= 1 << r
    return out


def docs_of(bits, act=None):
    act = active_docs() if act is None else act
    n = (len(act) + 7) // 8
    on = np.unpackbits(np.frombuffer(bits.to_bytes(n, "little"), dtype=np.uint8), bitorder="little")[: len(act)]
    return act[np.nonzero(on)[0]].astype(np.uint32)


def replay(nodes, leaf_bits, mutant=None, nbits=None):
    """tree_wide_fold over `nodes` (HostPlan.tree_nodes_wide: DevTreeNodeW) in Python integers, a bit per active document; leaf_bits: {term id: bits}.
    -> (the root's bits, the highest stack pointer reached).  mutant: one of MUTANTS, a deliberately WRONG fold — `thr_byte`: min(thr, 255), the narrow record's
    byte; `planes8`: cbits capped at 8; `stack32`: the slot mask one bit short; `nodes64`: the node count clamped to the narrow kernels' 64."""
    assert mutant is None or mutant in MUTANTS
    full = (1 << (len(active_docs()) if nbits is None else nbits)) - 1
    smask = 31 if mutant == "stack32" else 63
    planes = (lambda cb: min(cb, 8)) if mutant == "planes8" else (lambda cb: cb)
    stk = [0] * 64
    nn = min(len(nodes), 64) if mutant == "nodes64" else len(nodes)
    sp = high = m = 0
    for n in range(nn):
        x = nodes[n]
        op = int(x["op"])
        if op in (O.OP_TERM, O.OP_PHRASE):
            v = leaf_bits[int(x["arg"])]
        elif op == OP_SOME:
            cb, thr = planes(int(x["cbits"])), int(x["thr"])
            if mutant == "thr_byte":
                thr = min(thr, 255)
            gt, eq = 0, full
            for p in range(cb - 1, -1, -1):
                c = stk[(sp - cb + p) & smask]
                tb = full if (thr >> p) & 1 else 0
                gt |= eq & c & ~tb & full
                eq &= ~(c ^ tb) & full
            v = 0 if thr >> cb else gt | eq
            sp -= cb
        else:
            sp -= 1
            v = stk[sp & smask]
        if int(x["parent"]) == 0xFFFF:
            m = v
            continue
        order, pop, pcb = int(x["ord"]), int(x["pop"]), planes(int(x["pcbits"]))
        if order == 0:
            stk[sp & smask] = v
            if pop == OP_SOME:
                for p in range(1, pcb):
                    stk[(sp + p) & smask] = 0
                sp += pcb
            else:
                sp += 1
            high = max(high, sp)
        elif pop == OP_AND:
            stk[(sp - 1) & smask] &= v
        elif pop == OP_OR:
            stk[(sp - 1) & smask] |= v
        elif pop == OP_NOT:
            stk[(sp - 1) & smask] &= ~v & full
        elif pop == OP_SOME:
            carry = v
            for p in range(pcb):
                s = (sp - pcb + p) & smask
                t = stk[s] & carry
                stk[s] ^= carry
                carry = t
    return m, high


# ---- which leaves k_tree_leaves_wide scores: node values leaves-up, then "an iterator sits here" root-down, in place -----------------------------------
def reached(nodes, leaf_rows, mutant=None):
    """k_tree_leaves_wide's two passes over `nodes` with a boolean row per node (an entry per active document); leaf_rows: {term id: row}.  -> {leaf node: the
    documents on which the leaf is reached}, to be read on the root's matches only.  mutant `parent_word`: a parent in another 32-node word is read one word too low."""
    nn = len(nodes)
    par = nodes["parent"].astype(np.int64)
    kids = [[] for _ in range(nn)]
    for k in range(nn - 1):
        kids[par[k]].append(k)
    bit = [None] * nn
    for n in range(nn):
        x = nodes[n]
        op = int(x["op"])
        rows = [bit[k] for k in kids[n]]
        if op in (O.OP_TERM, O.OP_PHRASE):
            bit[n] = leaf_rows[int(x["arg"])]
        elif op == OP_AND:
            bit[n] = np.logical_and.reduce(rows)
        elif op == OP_OR:
            bit[n] = np.logical_or.reduce(rows)
        elif op == OP_SOME:
            bit[n] = np.sum(rows, axis=0) >= int(x["thr"])
        elif op == OP_NOT:
            bit[n] = rows[0] & ~rows[1]
        else:  # OPT
            bit[n] = rows[0]
    for n in range(nn - 1, -1, -1):
        if n == nn - 1:
            bit[n] = np.ones_like(bit[n])
            continue
        p, order, pop = int(par[n]), int(nodes[n]["ord"]), int(nodes[n]["pop"])
        if mutant == "parent_word" and p >> 5 != n >> 5 and p >= 32:
            p -= 32
        via = True if pop == OP_AND else bit[n] if pop in (OP_OR, OP_SOME) else order == 0 if pop == OP_NOT else (order == 0) | bit[n]
        bit[n] = bit[p] & via
    return {n: bit[n] for n in range(nn) if int(nodes[n]["op"]) in (O.OP_TERM, O.OP_PHRASE)}
