"""The percolator's contract in plain Python (a helper module: tests/test_perc_cases.py pins it to the reference's answers, the GPU tests compare the device
with it), the builders of the named cases, and the slicing of an oracle corpus into tri_perc_docs arrays.

A stored query is a postfix program (trinity_amd.tok); a document is {term: ascending positions} (an empty list: held, but in no phrase).  For ONE document
(percolator.cpp:9-137): TERM: the document holds it; AND / OR: all / any child; NOT(2): lhs and not rhs; NOT(1): not the operand; OPT(2): the main side;
SOME: at least `min` children; PHRASE: some position p != 0 of the first word has p + j among the positions of word j, for every j; the empty program: never."""
import numpy as np

import trinity_amd as T

NONE = 0xFFFFFFFF
PHRASE_PASS = 64  # csrc/k_perc.hpp PERC_PHRASE_PASS: positions of a phrase's first word a wave checks per pass
MUTANTS = ("opt_requires_optional", "not2_as_and", "phrase_as_and", "some_off_by_one")


def phrase_holds(doc, words):
    if any(w not in doc for w in words):
        return False
    sets = [set(doc[w]) for w in words]
    return any(p != 0 and all((p + j) in sets[j] for j in range(1, len(words))) for p in doc[words[0]])


def match_one(prog, doc, mutant=None):
    """Does the program hold on the document?  mutant: one of MUTANTS — a deliberately WRONG evaluator (the tests check that the cases tell it from the right one)."""
    st = []  # (value, the term of a TERM token)
    for t in prog:
        op, arg = int(t) >> 28, int(t) & 0x0FFFFFFF
        if op == T.OP_TERM:
            st.append((arg in doc, arg))
            continue
        n = arg & 0xFFFF if op == T.OP_SOME else arg
        kids = st[len(st) - n :]
        del st[len(st) - n :]
        vals = [v for v, _ in kids]
        if op == T.OP_PHRASE:
            v = all(vals) if mutant == "phrase_as_and" else phrase_holds(doc, [w for _, w in kids])
        elif op == T.OP_AND:
            v = all(vals)
        elif op == T.OP_OR:
            v = any(vals)
        elif op == T.OP_NOT:
            v = (not vals[0]) if n == 1 else (vals[0] and vals[1]) if mutant == "not2_as_and" else (vals[0] and not vals[1])
        elif op == T.OP_OPT:
            v = (vals[0] and vals[1]) if mutant == "opt_requires_optional" else vals[0]
        elif op == T.OP_SOME:
            v = sum(vals) >= (arg >> 16) + (1 if mutant == "some_off_by_one" else 0)
        else:
            raise ValueError("not an operator: %d" % op)
        st.append((v, None))
    return bool(st[0][0]) if st else False


def match_batch(programs, docs):
    """Per program the documents it holds on, as a Python integer (bit d = document d): the same contract over whole batches."""
    full = (1 << len(docs)) - 1
    holds, phrases = {}, {}
    for d, doc in enumerate(docs):
        for t in doc:
            holds[t] = holds.get(t, 0) | (1 << d)

    def phrase(words):
        if words not in phrases:
            cand, out = full, 0
            for w in words:
                cand &= holds.get(w, 0)
            while cand:
                low = cand & -cand
                if phrase_holds(docs[low.bit_length() - 1], words):
                    out |= low
                cand ^= low
            phrases[words] = out
        return phrases[words]

    out = []
    for prog in programs:
        st = []
        for t in prog:
            op, arg = int(t) >> 28, int(t) & 0x0FFFFFFF
            if op == T.OP_TERM:
                st.append((holds.get(arg, 0), arg))
                continue
            n = arg & 0xFFFF if op == T.OP_SOME else arg
            kids = st[len(st) - n :]
            del st[len(st) - n :]
            if op == T.OP_PHRASE:
                v = phrase(tuple(w for _, w in kids))
            elif op == T.OP_AND:
                v = full
                for k, _ in kids:
                    v &= k
            elif op == T.OP_OR:
                v = 0
                for k, _ in kids:
                    v |= k
            elif op == T.OP_NOT:
                v = full ^ kids[0][0] if n == 1 else kids[0][0] & ~kids[1][0]
            elif op == T.OP_OPT:
                v = kids[0][0]
            else:  # SOME: a bit-sliced count would do; the documents are few — count per threshold
                ge = [full] + [0] * n  # ge[c]: the documents on which at least c of the children seen so far hold
                for k, _ in kids:
                    for c in range(n, 0, -1):
                        ge[c] |= ge[c - 1] & k
                v = ge[arg >> 16]
            st.append((v, None))
        out.append(st[0][0] if st else 0)
    return out


def pairs_of(bits, ndocs):
    """((queries, docs) query-major, (queries, docs) document-major, per-document counts) of match_batch's answer."""
    nbytes = (ndocs + 7) // 8
    m = np.zeros((max(1, len(bits)), nbytes), dtype=np.uint8)
    for q, b in enumerate(bits):
        if b:
            m[q] = np.frombuffer(b.to_bytes(nbytes, "little"), dtype=np.uint8)
    on = np.unpackbits(m, axis=1, bitorder="little")[:, :ndocs]
    q1, d1 = np.nonzero(on)
    d2, q2 = np.nonzero(on.T)
    return (q1.astype(np.uint32), d1.astype(np.uint32)), (q2.astype(np.uint32), d2.astype(np.uint32)), on.sum(axis=0).astype(np.uint32)


def arrays_of(docs):
    """(doc_first, terms, freqs, positions) of a list of {term: positions} documents."""
    doc_first, terms, freqs, pos = [0], [], [], []
    for doc in docs:
        for t in sorted(doc):
            terms.append(t)
            freqs.append(len(doc[t]))
            pos.extend(doc[t])
        doc_first.append(len(terms))
    return np.array(doc_first, np.uint64), np.array(terms, np.uint32), np.array(freqs, np.uint32), np.array(pos, np.uint16)


def docs_of(doc_first, terms, freqs, positions):
    """The inverse: the documents the restatement reads."""
    out, at = [], 0
    for d in range(len(doc_first) - 1):
        doc = {}
        for i in range(int(doc_first[d]), int(doc_first[d + 1])):
            f = int(freqs[i])
            if int(terms[i]) != NONE:
                doc[int(terms[i])] = [int(p) for p in positions[at : at + f]]
            at += f
        out.append(doc)
    return out


def write_case_file(path, programs, docs):
    """The case file of the two C++ drivers (tests/cpp/perc_case_file.hpp): nq, per query its tokens; ndocs, per document its terms with their positions."""
    lines = [str(len(programs))] + [" ".join([str(len(p))] + [str(int(t)) for t in p]) for p in programs] + [str(len(docs))]
    for doc in docs:
        lines.append(" ".join([str(len(doc))] + [" ".join([str(t), str(len(doc[t]))] + [str(p) for p in doc[t]]) for t in sorted(doc)]))
    open(path, "w").write("\n".join(lines) + "\n")


def corpus_batch(corpus, ndocs):
    """Documents 1 .. ndocs of an oracle corpus (oracle_lib.ToCorpus: term_off / tok_doc / tok_pos, the tokens term-major) as a batch: document d of the
    batch is docID d + 1."""
    c = corpus.contents
    n, V = int(c.ntokens), int(c.V)
    off = np.ctypeslib.as_array(c.term_off, shape=(V + 1,)).astype(np.int64)
    doc = np.ctypeslib.as_array(c.tok_doc, shape=(n,)).astype(np.int64)
    pos = np.ctypeslib.as_array(c.tok_pos, shape=(n,)).astype(np.int64)
    term = np.repeat(np.arange(V, dtype=np.int64), np.diff(off))
    keep = doc <= ndocs
    doc, pos, term = doc[keep] - 1, pos[keep], term[keep]
    order = np.lexsort((pos, term, doc))
    doc, pos, term = doc[order], pos[order], term[order]
    key = doc * V + term
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    freqs = np.diff(np.r_[first, key.size])
    doc_first = np.searchsorted(doc[first], np.arange(ndocs + 1))
    return doc_first.astype(np.uint64), term[first].astype(np.uint32), freqs.astype(np.uint32), pos.astype(np.uint16)


def tk(*terms):
    return [T.tok(T.OP_TERM, t) for t in terms]


def phrase(*terms):
    return tk(*terms) + [T.tok(T.OP_PHRASE, len(terms))]


# ---- the named case families: (programs, documents, dictionary size).  Each holds a pair on which one of MUTANTS answers wrongly
def family_opt():
    progs = [tk(1, 2) + [T.tok(T.OP_OPT, 2)], tk(1) + tk(2, 3) + [T.tok(T.OP_OR, 2), T.tok(T.OP_OPT, 2)], tk(4) + tk(1, 2) + [T.tok(T.OP_OPT, 2), T.tok(T.OP_AND, 2)]]
    docs = [{1: [1]}, {1: [1], 2: [2]}, {2: [1]}, {1: [3], 4: [4]}, {}]
    return progs, docs, 8


def family_not():
    progs = [tk(1, 2) + [T.tok(T.OP_NOT, 2)], tk(1) + [T.tok(T.OP_NOT, 1)], tk(1, 2) + [T.tok(T.OP_OR, 2), T.tok(T.OP_NOT, 1)],
             tk(3) + tk(1) + [T.tok(T.OP_NOT, 1), T.tok(T.OP_AND, 2)], tk(1) + tk(2, 3) + [T.tok(T.OP_AND, 2), T.tok(T.OP_NOT, 2)]]  # fmt: skip
    docs = [{1: [1]}, {1: [1], 2: [2]}, {2: [1]}, {1: [1], 2: [2], 3: [3]}, {3: [9]}, {}]
    return progs, docs, 8


def family_some():
    progs = [tk(1, 2, 3) + [T.tok(T.OP_SOME, (m << 16) | 3)] for m in (1, 2, 3)]
    progs.append(tk(1) + tk(2, 3) + [T.tok(T.OP_AND, 2)] + tk(4, 5, 6) + [T.tok(T.OP_SOME, (3 << 16) | 5)])
    docs = [{1: [1]}, {1: [1], 2: [2]}, {1: [1], 2: [2], 3: [3]}, {2: [1], 3: [2], 4: [3]}, {1: [1], 4: [2], 5: [3]}, {}]
    return progs, docs, 8


def family_phrase():
    """Adjacent words; the same words out of order; a repeated word; a posting of frequency 0; position 0 on the first and on a later word; positions at the top of
    u16; a posting of PHRASE_PASS + 1 positions of which only the last starts the phrase; an empty document."""
    progs = [phrase(1, 2), phrase(1, 2, 3), phrase(4, 4), tk(1), tk(1, 2) + [T.tok(T.OP_AND, 2)], phrase(1, 2) + tk(3) + [T.tok(T.OP_NOT, 2)], phrase(2, 1),
             phrase(1, 2, 3, 5, 6, 7), phrase(1, 2) + [T.tok(T.OP_NOT, 1)]]  # fmt: skip
    docs = [
        {1: [5], 2: [6], 3: [7]},
        {1: [5], 2: [7], 3: [6]},
        {1: [0], 2: [1]},
        {1: [3], 2: [0]},
        {4: [2, 3]},
        {4: [2]},
        {1: [], 2: [6]},
        {1: [65534], 2: [65535]},
        {1: [65535], 2: [0]},
        {1: list(range(1, PHRASE_PASS + 2)), 2: [PHRASE_PASS + 2]},
        {},
        {1: [10], 2: [11], 3: [12], 5: [13], 6: [14], 7: [15]},
        {1: [10], 2: [11], 3: [12], 5: [13], 6: [15], 7: [14]},
        {1: [0, 4], 2: [1, 5]},
    ]
    return progs, docs, 8


FAMILIES = {"opt_requires_optional": family_opt, "not2_as_and": family_not, "phrase_as_and": family_phrase, "some_off_by_one": family_some}
