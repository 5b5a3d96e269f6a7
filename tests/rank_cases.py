"""The proximity ranker of the default mode (tri_batch_set_ranker, TRI_RANK_PROXIMITY) restated in plain Python over the CPU oracle's default mode — a helper
module, imported by tests/test_gpu_rank.py, tests/test_host_mirror_rank.py and tests/test_rank_cpu.py.  Nothing here comes from the engine: the matches, the
matched terms, their frequencies and positions are oracle_lib.Index.exec_rich's records; the slots come from the program's own token order; the arithmetic is
Python floats (IEEE double, one operation at a time), in the order the contract writes it."""

OP_TERM, OP_AND, OP_OR, OP_PHRASE, OP_NOT, OP_OPT, OP_SOME = range(7)


def reportable_tokens(prog):
    """Per token: True for a TERM token outside the excluded side of a NOT (the second operand's sub-program)."""
    prog = [int(x) for x in prog]
    rep = [(t >> 28) == OP_TERM for t in prog]
    start = []  # per sub-program on the evaluation stack: its first token
    for i, t in enumerate(prog):
        op, arg = t >> 28, t & 0x0FFFFFFF
        if op == OP_TERM:
            start.append(i)
            continue
        kids = arg if op in (OP_AND, OP_OR, OP_PHRASE) else (arg & 0xFFFF) if op == OP_SOME else 2
        if op == OP_NOT:
            for j in range(start[-1], i):
                rep[j] = False
        first = start[len(start) - kids]
        del start[len(start) - kids :]
        start.append(first)
    assert len(start) == 1
    return rep


def slots(prog):
    """-> (terms, tokens): slot k's term — the distinct terms that have a reportable token, in order of first appearance in the program (the order of
    tri_batch_query_terms) — and the index of the first reportable token that names it (where its weight is read)."""
    prog = [int(x) for x in prog]
    rep = reportable_tokens(prog)
    positive = {t & 0x0FFFFFFF for t, r in zip(prog, rep) if r}
    terms, toks = [], []
    for t in prog:
        x = t & 0x0FFFFFFF
        if (t >> 28) == OP_TERM and x in positive and x not in terms:
            terms.append(x)
            toks.append(next(i for i, (u, r) in enumerate(zip(prog, rep)) if r and (u & 0x0FFFFFFF) == x))
    return terms, toks


def token_weights(progs, fn):
    """One weight per token of the flattened programs: fn(slot) for the tokens that give a slot its weight, 0.0 elsewhere (never read)."""
    out = []
    for p in progs:
        w = [0.0] * len(p)
        for k, t in enumerate(slots(p)[1]):
            w[t] = float(fn(k))
        out += w
    return out


def records(flat):
    """exec_rich's flat stream -> [(doc, {term: (freq, [positions])})]"""
    flat = [int(x) for x in flat]
    out, i = [], 0
    while i < len(flat):
        doc, nt = flat[i], flat[i + 1]
        i += 2
        terms = {}
        for _ in range(nt):
            t, f = flat[i], flat[i + 1]
            terms[t] = (f, flat[i + 2 : i + 2 + f])
            i += 2 + f
        out.append((doc, terms))
    return out


def pairs_of(terms, slot_terms):
    n = 0
    for k in range(len(slot_terms) - 1):
        a, b = terms.get(slot_terms[k]), terms.get(slot_terms[k + 1])
        if a is None or b is None:
            continue
        nxt = set(b[1])
        n += sum(1 for h in a[1] if h != 0 and h + 1 in nxt)
    return n


def score(terms, slot_terms, w, freq_cap, adjacency):
    s = 0.0
    for k, t in enumerate(slot_terms):
        if t in terms:
            s += w[k] * float(min(terms[t][0], freq_cap))
    return s + adjacency * float(pairs_of(terms, slot_terms))


def rows(recs, prog, freq_cap, adjacency, weights=None):
    """The whole ranking of one query from its records (records(flat)): [(docID, score, pairs)], score descending, docID ascending.  weights: per token of THIS
    program (None: 1.0)."""
    slot_terms, toks = slots(prog)
    w = [1.0 if weights is None else float(weights[t]) for t in toks]
    out = []
    for doc, terms in recs:
        out.append((doc, score(terms, slot_terms, w, freq_cap, adjacency), pairs_of(terms, slot_terms)))
    return sorted(out, key=lambda r: (-r[1], r[0]))


def ranked(flat, prog, K, freq_cap, adjacency, weights=None):
    """The expected list of one query: ([docIDs], [scores], [pairs]) of its best K matches."""
    r = rows(records(flat), prog, freq_cap, adjacency, weights)[:K]
    return [x[0] for x in r], [x[1] for x in r], [x[2] for x in r]
