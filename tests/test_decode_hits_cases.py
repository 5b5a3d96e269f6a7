"""The cases of tests/decode_hits_cases.py reach the boundaries they are there for — checked on the encoded bytes through the upload walk (hostplan.HostIndex:
block counts, the BLK_HITS_PLAIN bits, hdir's full 128-hit groups) —, the binding and the C++ mirror of the hit decode exist and link, and the mirror's
DocWordsSpace behaves as docwordspace.h's under ASan + UBSan.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import decode_hits_cases as DC
import oracle_lib as O
import structured as S


@pytest.fixture(scope="module")
def T():
    import trinity_amd

    trinity_amd.build_all()
    return trinity_amd


@pytest.fixture(scope="module")
def c(T):
    return DC.corpus()


def _dirs(c, name):
    t = c.tid[name]
    g, _ = c.host_index(1).hits_dir(t)
    l, nfull = c.host_index(2).hits_dir(t)
    return g, l, nfull


def test_split_threshold_mirror():
    k = S.header_constants("dev_structs.hpp", "k_decode_hits.hpp")
    assert k["DH_SPLIT"] == DC.DH_SPLIT and k["BLK_HITS_PLAIN"] == DC.BLK_HITS_PLAIN


def test_document_counts_reach_the_block_ends(c):
    for n in DC.DOC_COUNTS:
        g, l, nfull = _dirs(c, f"n{n}")
        blocks = S.google_blocks(c.g_index, c.g_terms, c.tid[f"n{n}"])
        assert len(g) == len(l) == len(blocks) == (n + 31) // 32, n
        assert [b[1] for b in blocks] == [32] * (n // 32) + ([n % 32] if n % 32 else []), n
        assert nfull == n // 128 and np.all(g >> 31 == 1), n  # frequency 1: hits = documents; every block plain
        # LUCENE: the rows' hit ordinals are the documents before them
        assert l.tolist() == [32 * b for b in range(len(l))], n
    assert (32 * 256 + 5 + 31) // 32 > 256  # past one workgroup's chunk of 256 blocks
    assert {n % 128 for n in DC.DOC_COUNTS} >= {0, 1, 127}  # with and without a varbyte tail of documents


def test_hit_totals_reach_the_group_ends(c):
    for h in DC.HIT_TOTALS:
        _, l, nfull = _dirs(c, f"h{h}")
        assert int(c.lists[f"h{h}"][1].sum()) == h == c.positions[f"h{h}"].size and nfull == h // 128, h
    assert {h % 128 for h in DC.HIT_TOTALS} >= {0, 1, 127}
    g, l, nfull = _dirs(c, "ones")
    assert nfull == 2 and np.all(c.positions["ones"] == 1) and np.all(c.lists["ones"][1] == 1)


def test_long_documents_sit_where_they_should(c):
    for name, before, big in (("at100", 100, 200), ("at90", 90, 100)):
        d, f = c.lists[name]
        k = int(np.argmax(f))
        assert int(f[k]) == big and int(f[:k].sum()) == before and before < 128 < before + big  # it straddles the first hit group's end
        assert (big > DC.DH_SPLIT) == (name == "at100")
        assert _dirs(c, name)[2] == (before + big + 40) // 128
    d, f = c.lists["mid300"]
    assert f.tolist() == [1] * 10 + [300] + [1] * 10 and len(_dirs(c, "mid300")[0]) == 1 and 300 > DC.DH_SPLIT  # one GOOGLE block
    assert (c.lists["zeros"][1] == 0).sum() == 40 and c.lists["empty"][0].size == 0
    assert len(_dirs(c, "empty")[0]) == 0


def test_position_deltas_turn_plain_off_for_their_block_only(c):
    for k in DC.DELTAS:
        g, _, _ = _dirs(c, f"d{k}")
        assert (g >> 31).tolist() == ([1, 1, 1] if k < 64 else [1, 0, 1]), k
    # prefix varint of (delta << 1): one byte below 128, two below 16384, then three
    vb = lambda v: 1 if v < 0x80 else 2 if v < 0x4000 else 3  # noqa: E731
    assert [vb(k << 1) for k in DC.DELTAS] == [1, 2, 2, 3]
    g, _, _ = _dirs(c, "last")
    assert int(c.positions["last"].max()) == 16383 and (g >> 31).tolist() == [0]


def test_payload_case_has_the_length_changes(T):
    index, terms, docs_cnt, postings, hits = DC.payload_case()
    ora = O.Index.wrap(index, terms, docs_cnt, postings, hits)
    f, p, ln, w = DC.oracle_hits(ora, 0)
    assert ln[:5].tolist() == [0, 3, 8, 1, 0] and ln[5:8].tolist() == [8, 8, 2] and ln[8] == 0  # inside a document; restart after a document that ended on a payload
    assert int(w[3]) >> 8 == int(w[2]) >> 8 and int(w[3]) != int(w[2])  # a 1-byte payload over an 8-byte one: stale high bytes
    f1, _, ln1, w1 = DC.oracle_hits(ora, 1)
    assert f1.size == 40 and np.all(ln1 == 4) and np.all(w1 < 1 << 32)  # constant over a full block and a short one
    _, _, ln2, _ = DC.oracle_hits(ora, 2)
    assert not ln2.any()
    from trinity_amd import hostplan as HP

    h = HP.HostIndex(index, terms, docs_cnt)
    assert not (h.hits_dir(0)[0] >> 31).any() and not (h.hits_dir(1)[0] >> 31).any() and (h.hits_dir(2)[0] >> 31).all()


def test_binding_and_mirror_exist_and_link(T):
    from trinity_amd.build import LIB_HIP, MIRROR_HITS_BIN

    assert callable(T.Index.decode_hits) and callable(T.Index.decode_hits_at)
    assert {"tri_decode_hits", "tri_decode_hits_at"} <= set(T.engine.ABI_SYMBOLS)
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB_HIP], capture_output=True, text=True).stdout
    assert re.search(r" T tri_decode_hits$", syms, re.M) and re.search(r" T tri_decode_hits_at$", syms, re.M)
    assert os.path.exists(MIRROR_HITS_BIN)
    assert "libtrinity_hip.so" in subprocess.run(["ldd", MIRROR_HITS_BIN], capture_output=True, text=True).stdout


DWS_MAIN = r"""
#include "trinity_gpu.hpp"
#include <cstdio>
using namespace trinity_amd;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
        DocWordsSpace s;
        EXPECT(s.max_pos() == 16383);
        EXPECT(!s.test(1, 5));
        s.set(1, 5);
        EXPECT(s.test(1, 5) && !s.test(2, 5) && !s.test(1, 4) && !s.test(1, 6));
        s.set(2, 5); // one term per position: the last writer wins
        EXPECT(s.test(2, 5) && !s.test(1, 5));
        s.set(7, 16383);
        s.set(9, 65535); // any tokenpos_t is a cell ...
        EXPECT(s.test(7, 16383) && s.test(9, 65535));
        for (uint32_t k = 1; k <= 16; ++k) // ... and a phrase test may look MaxPhraseSize past it
                EXPECT(!s.test(9, 65535u + k));
        EXPECT(!s.test(0, 0)); // position 0 is never set: a fresh cell is nobody's
        s.unset(16383);
        EXPECT(!s.test(7, 16383));
        s.reset();
        EXPECT(!s.test(2, 5) && !s.test(9, 65535));
        s.set(3, 5);
        EXPECT(s.test(3, 5));
        for (int i = 0; i < 70000; ++i) { // across the sequence number's wrap: what an earlier document wrote never comes back
                s.reset();
                EXPECT(!s.test(3, 5) && !s.test(4, 6));
                if (i % 1000 == 0)
                        s.set(4, 6), s.set(3, 5);
        }
        s.set(5, 1);
        EXPECT(s.test(5, 1));
        try {
                DocWordsSpace bad(0);
                EXPECT(false);
        } catch (const invalid_argument &) {
        }
        printf("OK\n");
        return 0;
}
"""


def test_docwordsspace_under_sanitizers(T, tmp_path):
    """A stand-alone program (its own main, run directly) around the mirror's DocWordsSpace, compiled with -fsanitize=address,undefined.  The header's
    other classes reference the engine's C-ABI, so the program links to the library; it calls nothing of it and touches no device.  The
    sanitizers' runtimes are linked statically: the program is then checked whatever the environment preloads."""
    src = tmp_path / "dws_main.cpp"
    src.write_text(DWS_MAIN)
    exe = tmp_path / "dws_main"
    inc = os.path.join(O.ROOT, "trinity_amd", "csrc", "host")
    lib = os.path.join(O.ROOT, "trinity_amd")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-I" + inc, "-o", str(exe), str(src),
                    "-L" + lib, "-ltrinity_hip", "-Wl,-rpath," + lib], check=True)  # fmt: skip
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "OK", res.stdout[-2000:] + res.stderr[-2000:]
