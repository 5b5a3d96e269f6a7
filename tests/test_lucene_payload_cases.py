"""Hit payloads in the Lucene-shaped codec on the CPU (tests/lucene_payload_cases.py is the restatement):

  * the restated reader gives back what the restated writer was given, on every family, and each deliberately wrong reader is told from it by the family named for it;
  * the sequential host encoder (csrc/host/lucene_encoder.hpp), the device encoder's units run in plain loops (csrc/lucene_enc_units.hpp) and the restated writer give
    the same `index`, `hits.data` and term table on every family; with no payload arrays — and with all-zero lengths — the bytes are the payload-less exports';
  * the term header's chunk size and the skiplist's hit-block offsets count the payload bytes;
  * the upload walk (csrc/index_host.hpp) accepts every family, flags exactly the terms that carry a payload, and its payload directory points where the restated walk
    stands — also on the image the FastPFor transcoder leaves —, and refuses a length of 9, a block whose byte count disagrees with its lengths, a tail whose payload bytes
    overrun the chunk and stray bytes behind the tail;
  * a stand-alone program (tests/cpp/lucene_payload_test.cpp, g++ -fsanitize=address,undefined) runs the host encoder, the units and the upload walk over case files written
    from the same families and refusals."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import lucene_payload_cases as LP
import oracle_lib as O
import trinity_amd as T
from trinity_amd import hostplan as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(LP.FAMILIES)


@pytest.fixture(scope="module", autouse=True)
def built():
    T.build.build_host()
    O.lib()


@pytest.fixture(scope="module")
def written():
    made = {}

    def get(name):
        if name not in made:
            postings = LP.FAMILIES[name]()
            made[name] = (postings, LP.write(postings))
        return made[name]

    return get


def u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def host_index(index, hits, table):
    return HP.HostIndex(u8(index), np.array(table, dtype=np.uint32).reshape(-1, 3), 1 << 20, codec=2, hits=u8(hits))


@pytest.mark.parametrize("name", NAMES)
def test_the_reader_returns_what_the_writer_was_given(written, name):
    postings, (index, hits, table) = written(name)
    assert LP.read(index, hits, table) == LP.expected(postings)


@pytest.mark.parametrize("mutant", LP.MUTANTS)
def test_each_wrong_reader_is_caught_by_its_family(written, mutant):
    postings, (index, hits, table) = written(LP.CATCHES[mutant])
    assert LP.read(index, hits, table) == LP.expected(postings)
    assert LP.read(index, hits, table, mutant=mutant) != LP.expected(postings)


def test_the_agreement_rule_is_the_carry_rule(written):
    """agree_with_google() is exactly: the reader that carries the word's high bytes answers the same."""
    seen = set()
    for name in NAMES:
        postings, (index, hits, table) = written(name)
        same = LP.read(index, hits, table, mutant="carry_high_bytes") == LP.expected(postings)
        assert same == LP.agree_with_google(postings), name
        seen.add(same)
    assert seen == {True, False}


def test_the_families_hold_the_shapes_they_name(written):
    sizes = [sum(len(h) for _, h in term) for term in LP.hits_at_block_edges()]
    assert sizes == [127, 128, 129, 255, 256, 257]
    # the length groups of length_group_shapes: the all-equal form, today's three bytes, width 0 plus exceptions, width 4; byte counts in both varint classes
    _, (index, hits, table) = written("length_group_shapes")
    at, shapes, counts = 0, [], []
    for _ in range(4):
        _, at = LP.ints_get(hits, at)
        first = hits[at]
        w0 = int.from_bytes(hits[at + 1 : at + 5], "little")
        shapes.append("equal" if first == 0 else (w0 & 0xFF, (w0 >> 8) & 0xFF))
        _, at = LP.ints_get(hits, at)
        n, after = LP.varbyte_get(hits, at)
        counts.append((n, after - at))
        at = after + n
    assert shapes[0] == "equal" and shapes[1] == "equal" and shapes[2] == (0, 5) and shapes[3][0] == 4 and shapes[3][1] == 0
    assert counts[0] == (1024, 2) and counts[1] == (0, 1) and counts[2] == (40, 1)
    # the tail whose second document's first hit carries no flag
    _, (index, hits, table) = written("tail_state_runs_across_documents")
    assert hits[:2] == bytes([1 << 1 | 1, 3]) and hits[2:5] == bytes([1 << 1, 1 << 1, 1 << 1])  # (positions 1, 2 | 1, 2: the second document's first delta is 1, flag 0)
    # 129 document blocks
    postings, (index, hits, table) = written("skiplist_past_payload_blocks")
    assert table[0][0] // 128 == 129 and len(LP.skiplist(index, table[0])) == 129


@pytest.mark.parametrize("name", NAMES)
def test_host_encoder_and_units_write_the_restated_bytes(written, name):
    postings, (index, hits, table) = written(name)
    d, f, p, pl, pv, tf = LP.arrays(postings)
    for units in (False, True):
        gi, gh, gt = HP.lucene_encode(d, f, p, tf, units=units, payload_lens=pl, payloads=pv)
        assert [tuple(r) for r in gt.tolist()] == table, (name, units)
        assert gi.tobytes() == index, (name, units, "index")
        assert gh.tobytes() == hits, (name, units, "hits.data")


@pytest.mark.parametrize("name", NAMES)
def test_without_payloads_the_bytes_are_the_payloadless_exports(written, name):
    """No arrays, and arrays of zero lengths, against the exports that take no payloads — and against the restated writer over the same postings without payloads."""
    postings, _ = written(name)
    bare = [[(doc, [(pos, 0, 0) for pos, _, _ in doc_hits if pos]) for doc, doc_hits in term] for term in postings]
    d, f, p, pl, pv, tf = LP.arrays(bare)
    index, hits, table = LP.write(bare)
    for units in (False, True):
        plain = HP.lucene_encode(d, f, p, tf, units=units)
        zeros = HP.lucene_encode(d, f, p, tf, units=units, payload_lens=pl, payloads=pv)
        for a, b in zip(plain, zeros):
            assert np.array_equal(a, b), (name, units)
        assert plain[0].tobytes() == index and plain[1].tobytes() == hits, (name, units)


def test_chunk_sizes_and_skiplist_offsets_count_the_payload_bytes(written):
    for name in NAMES:
        postings, (index, hits, table) = written(name)
        end = 0
        for term, entry in zip(postings, table):
            docs, (hits_off, sum_hits, chunk, nskip) = LP.read_documents(index, entry)
            assert hits_off == end  # (the terms' chunks tile hits.data)
            end = hits_off + chunk
            # where every full hit block starts, by walking the chunk
            starts, at = [], hits_off
            for _ in range(sum_hits // 128):
                starts.append(at - hits_off)
                _, at = LP.ints_get(hits, at)
                lens, at = LP.ints_get(hits, at)
                n, at = LP.varbyte_get(hits, at)
                assert n == sum(lens)
                at += n
            starts.append(at - hits_off)
            before = np.concatenate([[0], np.cumsum([f for _, f in docs])])
            for j, e in enumerate(LP.skiplist(index, entry)):
                hb = int(before[128 * j])
                assert e[2] == starts[hb // 128] and e[4] == hb // 128 * 128 and e[5] == hb % 128 and e[3] == 128 * j, (name, j)
        assert end == len(hits)


@pytest.mark.parametrize("name", NAMES)
def test_upload_walk_flags_the_terms_and_points_at_their_payloads(written, name):
    postings, (index, hits, table) = written(name)
    H = host_index(index, hits, table)
    for t, (term, entry) in enumerate(zip(postings, table)):
        carries = any(length for _, doc_hits in term for _, length, _ in doc_hits)
        pd = H.payload_dir(t)
        assert (pd is not None) == carries, (name, t)
        if not carries:
            continue
        rows, tail_at = pd
        _, (hits_off, sum_hits, chunk, _) = LP.read_documents(index, entry)
        at = hits_off
        assert rows.shape[0] == sum_hits // 128
        for row in rows.tolist():
            _, at = LP.ints_get(hits, at)
            assert row[0] == at  # the length group
            lens, at = LP.ints_get(hits, at)
            _, at = LP.varbyte_get(hits, at)
            assert row[1] == at  # the payload bytes
            q = np.cumsum(lens)[[31, 63, 95]].tolist()
            assert row[2] == q[0] | q[1] << 10 | q[2] << 20
            at += sum(lens)
        tail_bytes = sum(h[1] for h in LP.read_hit_stream(hits, hits_off, sum_hits, chunk)[sum_hits // 128 * 128 :])
        assert tail_at == hits_off + chunk - tail_bytes


def test_upload_walk_through_the_fastpfor_container(written):
    """The same postings with FastPFor<4> words in the ints() groups (the container restated; the words from csrc/fastpfor128.hpp): the walk sees the transcoded image,
    and its directory points into THAT image — the payload bytes it points at are the hits' payloads."""
    postings = LP.fastpfor_postings()
    index, hits, table = LP.write_fastpfor(postings)
    pindex, phits, ptable = LP.write(postings)
    assert hits != phits
    H = host_index(index, hits, table)
    info = np.zeros(6, dtype=np.uint64)
    per = np.zeros((len(table), 3), dtype=np.uint32)
    HP._lib().tri_host_index_facts(C.c_void_p(H.h), C.c_void_p(info.ctypes.data), C.c_void_p(per.ctypes.data))
    assert info[4] > 0  # groups were transcoded
    P = host_index(pindex, phits, ptable)
    for t in range(len(table)):
        a, b = H.payload_dir(t), P.payload_dir(t)
        assert a is not None and np.array_equal(a[0], b[0]) and a[1] == b[1], t  # the transcoded image is the PFOR128 one


@pytest.mark.parametrize("name", sorted(LP.refusals()))
def test_upload_walk_refuses(name):
    index, hits, table, word = LP.refusals()[name]
    with pytest.raises(T.TrinityError, match=word):
        host_index(index, hits, table)


def test_host_encoder_refuses_a_payload_of_nine_bytes():
    d, f, p, pl, pv, tf = LP.arrays([[(1, [(1, 8, 5), (2, 3, 5)])]])
    pl[1] = 9
    with pytest.raises(T.TrinityError, match="refuses"):
        HP.lucene_encode(d, f, p, tf, payload_lens=pl, payloads=pv)


# ---- the stand-alone program under the sanitizers ----------------------------------------------------------------------------------------------------
def case_file(path, arrays, index, hits, table, refuse):
    """u32 magic, u32 refuse (0: encode and upload; 1: the upload must refuse these bytes), then the arrays and the expected bytes, each as u64 count + data."""
    d, f, p, pl, pv, tf = arrays
    with open(path, "wb") as out:
        out.write(struct.pack("<II", 0x5041594C, refuse))
        for a in (d, f, p, pl, pv, tf, u8(index), u8(hits), np.array(table, dtype=np.uint32).reshape(-1)):
            a = np.ascontiguousarray(a)
            out.write(struct.pack("<Q", a.size))
            out.write(a.tobytes())


def test_standalone_program_under_the_sanitizers(written, tmp_path):
    exe = str(tmp_path / "lucene_payload_test")
    src = os.path.join(ROOT, "tests", "cpp", "lucene_payload_test.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", exe, src],
                   check=True)  # fmt: skip
    files = []
    for name in NAMES:
        postings, (index, hits, table) = written(name)
        files.append(str(tmp_path / f"{name}.case"))
        case_file(files[-1], LP.arrays(postings), index, hits, table, 0)
    empty = LP.arrays([])
    for name, (index, hits, table, _) in LP.refusals().items():
        files.append(str(tmp_path / f"refuse_{name}.case"))
        case_file(files[-1], empty, index, hits, table, 1)
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(files)} cases" in r.stdout
