"""How the radius lists of W row shards become one list per query (pn_sharded_query_radius_*, the radius self-queries),
asked on the CPU: tests/cpp/csr_splice.cpp includes csrc/csr_splice.h alone (host code, no HIP), is compiled with
g++ -std=c++17 -Wall -Werror under AddressSanitizer + UndefinedBehaviorSanitizer, and prints what the parts splice to.

The expected lists were derived BY HAND from the rule as radius_splice and self_splice of csrc/sharded.hip stated it
before it moved into csr_splice.h (commit 83b1912), never by running the new function.  Per query q over parts 0 .. W - 1,
part r holding the entries [off[q], off[q + 1]) of its arrays:
  not sorted: the parts' lists one after the other in part order, distances carried along;
  sorted:     each part's list is sorted by (distance, global row); repeatedly, of the parts' current heads, the first
              part in part order is the candidate and a later part r replaces it when
              d < db or (d == db and row < rowb) -- so -0.0 ties with +0.0 and the lower row goes first;
  self form:  the entries whose row equals the query's own row g0 + t are left out and the count is of what was kept;
  sizing:     the result holds sum over parts of off[nq] - off[0] entries at most (a part's offsets need not start at 0).
Worked through for "sorted_tie_across_parts": heads (0.0, 40) and (0.0, 8500) tie, 40 < 8500: 40; then (0.5, 7) against
(0.0, 8500): 8500; against (0.0, 8501): 8501; against (0.25, 9000): 9000; part 2 is exhausted: 7.  The program's input
arrays are heap allocations of exactly their length and its output arrays of exactly the sizing rule's, so a read or a
write past an end fails under the sanitizer."""
import os
import struct
import subprocess

import pytest

from conftest import ROOT

NZ = -0.0
FILL = (999, 9.0)  # entries in front of a part's first offset: never read

# name: (sorted, with distances, q0, m or None for the whole batch, g0 or None for "drop nothing",
#        parts [(offsets, [(row, distance)])]), expected per query [(row, distance)]
CASES = {
    "one_part_unsorted_rows_only": (
        (0, 0, 0, None, None, [([0, 2, 2, 3], [(3, 0), (9, 0), (4, 0)])]),
        [[(3, 0), (9, 0)], [], [(4, 0)]]),
    "one_part_sorted": (
        (1, 1, 0, None, None, [([0, 2, 3], [(5, 0.25), (2, 0.5), (7, 1.0)])]),
        [[(5, 0.25), (2, 0.5)], [(7, 1.0)]]),
    # W = 3, the middle part empty, query 1 empty in every part
    "three_parts_empty_middle_unsorted": (
        (0, 0, 0, None, None, [([0, 1, 1, 2], [(1, 0), (2, 0)]), ([0, 0, 0, 0], []), ([0, 2, 2, 2], [(20, 0), (21, 0)])]),
        [[(1, 0), (20, 0), (21, 0)], [], [(2, 0)]]),
    # 0.25 of part 2 before 0.5 of part 0 before 0.75 of part 2
    "three_parts_empty_middle_sorted": (
        (1, 1, 0, None, None, [([0, 1, 1, 2], [(1, 0.5), (2, 0.25)]), ([0, 0, 0, 0], []),
                               ([0, 2, 2, 2], [(20, 0.25), (21, 0.75)])]),
        [[(20, 0.25), (1, 0.5), (21, 0.75)], [], [(2, 0.25)]]),
    # part order, the distances travel with their rows and are not looked at
    "unsorted_with_distances": (
        (0, 1, 0, None, None, [([0, 2, 3], [(1, 0.5), (4, 0.25), (2, 1.0)]), ([0, 1, 3], [(10, 0.75), (11, 0.25), (15, 0.5)])]),
        [[(1, 0.5), (4, 0.25), (10, 0.75)], [(2, 1.0), (11, 0.25), (15, 0.5)]]),
    "sorted_tie_across_parts": (
        (1, 1, 0, None, None, [([0, 2], [(40, 0.0), (7, 0.5)]), ([0, 0], []),
                               ([0, 3], [(8500, 0.0), (8501, 0.0), (9000, 0.25)])]),
        [[(40, 0.0), (8500, 0.0), (8501, 0.0), (9000, 0.25), (7, 0.5)]]),
    "sorted_tie_own_row_dropped": (
        (1, 1, 0, 1, 8500, [([0, 2], [(40, 0.0), (7, 0.5)]), ([0, 0], []),
                            ([0, 3], [(8500, 0.0), (8501, 0.0), (9000, 0.25)])]),
        [[(40, 0.0), (8501, 0.0), (9000, 0.25), (7, 0.5)]]),
    "own_row_absent_nothing_dropped": (
        (1, 1, 0, 1, 123, [([0, 2], [(40, 0.0), (7, 0.5)]), ([0, 0], []),
                           ([0, 3], [(8500, 0.0), (8501, 0.0), (9000, 0.25)])]),
        [[(40, 0.0), (8500, 0.0), (8501, 0.0), (9000, 0.25), (7, 0.5)]]),
    # query 0: -0.0 at row 9 of part 0 against +0.0 at rows 3 and 12 of part 1: all tie, by row 3, 9, 12, then 0.25;
    # query 1: +0.0 at row 9 of part 0 against -0.0 at row 3 of part 1: tie, row 3 first.  Every sign as it came in.
    "negative_zero_ties_with_zero": (
        (1, 1, 0, None, None, [([0, 2, 3], [(9, NZ), (1, 0.25), (9, 0.0)]), ([0, 2, 3], [(3, 0.0), (12, 0.0), (3, NZ)])]),
        [[(3, 0.0), (9, NZ), (12, 0.0), (1, 0.25)], [(3, NZ), (9, 0.0)]]),
    # part 0 starts at entry 3 of its arrays, part 1 at entry 2: (6 - 3) + (3 - 2) = 4 entries
    "offsets_not_from_zero_unsorted": (
        (0, 1, 0, None, None, [([3, 4, 6], [FILL] * 3 + [(5, 0.5), (6, 0.25), (8, 1.0)]), ([2, 2, 3], [FILL] * 2 + [(70, 0.75)])]),
        [[(5, 0.5)], [(6, 0.25), (8, 1.0), (70, 0.75)]]),
    "offsets_not_from_zero_sorted": (
        (1, 1, 0, None, None, [([3, 4, 6], [FILL] * 3 + [(5, 0.5), (6, 0.25), (8, 1.0)]), ([2, 2, 3], [FILL] * 2 + [(70, 0.75)])]),
        [[(5, 0.5)], [(6, 0.25), (70, 0.75), (8, 1.0)]]),
    # the self form: queries 2 and 3 of a batch of 5 are rows 100 and 101.  Query 2: (100, 0.0) is its own, then (1, 0.25)
    # ties with (101, 0.25): row 1; (3, 0.5) against (101, 0.25): 101; then 3.  Query 3: (101, 0.0) is its own, (100, 0.25)
    # before (2, 0.5).
    "self_form_from_query_2_sorted": (
        (1, 1, 2, 2, 100, [([0, 1, 2, 4, 5, 6], [(0, 0.0), (1, 0.0), (1, 0.25), (3, 0.5), (2, 0.5), (0, 1.0)]),
                           ([0, 0, 1, 3, 5, 5], [(100, 0.5), (100, 0.0), (101, 0.25), (101, 0.0), (100, 0.25)])]),
        [[(1, 0.25), (101, 0.25), (3, 0.5)], [(100, 0.25), (2, 0.5)]]),
    "self_form_from_query_2_unsorted_rows_only": (
        (0, 0, 2, 2, 100, [([0, 1, 2, 4, 5, 6], [(0, 0), (1, 0), (1, 0), (3, 0), (2, 0), (0, 0)]),
                           ([0, 0, 1, 3, 5, 5], [(100, 0), (100, 0), (101, 0), (100, 0), (101, 0)])]),
        [[(1, 0), (3, 0), (101, 0)], [(2, 0), (100, 0)]]),
    # the same queries with nothing dropped (PN_SELF_INCLUDE)
    "self_form_from_query_2_included": (
        (0, 0, 2, 2, None, [([0, 1, 2, 4, 5, 6], [(0, 0), (1, 0), (1, 0), (3, 0), (2, 0), (0, 0)]),
                            ([0, 0, 1, 3, 5, 5], [(100, 0), (100, 0), (101, 0), (100, 0), (101, 0)])]),
        [[(1, 0), (3, 0), (100, 0), (101, 0)], [(2, 0), (100, 0), (101, 0)]]),
}


def _bits(bits, d):
    return struct.unpack("<I", struct.pack("<f", d))[0] if bits == 32 else struct.unpack("<Q", struct.pack("<d", d))[0]


def _input_line(bits, case):
    srt, wd, q0, m, g0, parts = case
    nq = len(parts[0][0]) - 1
    words = [bits, len(parts), nq, srt, wd, q0, nq if m is None else m, 0 if g0 is None else 1, g0 or 0]
    for off, entries in parts:
        assert len(off) == nq + 1 and off[-1] == len(entries)
        words += off + [len(entries)] + [r for r, _ in entries]
        if wd:
            words += ["%x" % _bits(bits, d) for _, d in entries]
    return " ".join(str(w) for w in words)


def _want_line(bits, case, lists):
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    rows = "".join(" %d" % r for l in lists for r, _ in l)
    dist = "".join(" %x" % _bits(bits, d) for l in lists for _, d in l) if case[1] else ""
    return " ".join(str(o) for o in off) + " |" + rows + " |" + dist


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the program, built under both sanitizers: a machine without their runtime fails here, it is never run unchecked"""
    out = str(tmp_path_factory.mktemp("splice") / "csr_splice")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "csr_splice.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_the_header_compiles_alone_with_plain_gxx(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(ROOT, "petal-neighbors_amd", "csrc", "csr_splice.h"))
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("bits", [32, 64])
def test_splices_equal_the_hand_derived_table(exe, bits):
    names = sorted(CASES)
    text = "\n".join(_input_line(bits, CASES[n][0]) for n in names) + "\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(names)
    wrong = []
    for line, name in zip(got, names):
        want = _want_line(bits, *CASES[name])
        if line != want:
            wrong.append((name, line, want))
    assert not wrong, wrong


def test_the_table_is_well_formed():
    """(of the table itself: offsets ascend, every kept entry is an entry of the spliced queries, a sorted part's lists
    are sorted, and what is missing from the expectation is exactly the own rows)"""
    for name, ((srt, wd, q0, m, g0, parts), lists) in CASES.items():
        nq = len(parts[0][0]) - 1
        m = nq if m is None else m
        assert len(lists) == m and q0 + m <= nq, name
        for t, kept in enumerate(lists):
            have = []
            for off, entries in parts:
                assert all(a <= b for a, b in zip(off, off[1:])), name
                mine = entries[off[q0 + t]:off[q0 + t + 1]]
                if srt:
                    assert mine == sorted(mine, key=lambda e: (e[1], e[0])), name
                have += mine
            own = None if g0 is None else g0 + t
            key = lambda e: (e[0], struct.pack("<d", e[1]))
            assert sorted(kept, key=key) == sorted([e for e in have if e[0] != own], key=key), name
            if srt:
                assert [(d, r) for r, d in kept] == sorted((d, r) for r, d in kept), name
