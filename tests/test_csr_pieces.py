"""Where a counted CSR is cut into pieces (DBSCAN, OPTICS, KDE and mean shift ask for their radius lists piece by piece),
asked on the CPU: tests/cpp/csr_pieces.cpp includes csrc/csr_pieces.h alone (host arithmetic, no HIP), is compiled with
g++ -std=c++17 -Wall -Werror under AddressSanitizer + UndefinedBehaviorSanitizer, and prints the pieces it walks through.

The expected pieces were derived BY HAND from the rule as the four entry points stated it before it moved into
csr_pieces.h (dbscan_enqueue, optics_enqueue, kde_enqueue and ms_enqueue of csrc/index.hip at commit b877b24), never by
running the new function.  From row a of off[0 .. n]:
  lim = min(n, a + chunk)
  b   = the last index in (a, lim] with off[b] - off[a] <= E
  b   = a + 1 where there is none (a single row longer than E is a piece of its own)
and the next piece starts at b.  Rows are given by their lengths; the offsets are their running sum from ``base``.  Worked
through for "exactly_E_and_E_plus_1" (E = 6, lengths 1 2 3 4 2 1, offsets 0 1 3 6 10 12 13): from 0, off[3] = 6 <= 6 and
off[4] = 10 > 6: b = 3, a piece of exactly E; from 3, off[5] - 6 = 6 <= 6 and off[6] - 6 = 7 = E + 1: b = 5; then 5:6.
Trailing empty rows belong to the piece before them (b is the LAST index within E), and empty rows in front of a row
longer than what is left of E form a piece without entries, which mean shift visits and the others skip."""
import os
import subprocess

import pytest

from conftest import ROOT

E_MAX = 2 ** 63 - 1  # the largest value pn_index_set_option accepts (an int64)

# name: (chunk, E, base, row lengths), pieces
CASES = {
    # E = 1: a row of one entry cannot take a non-empty neighbour along, a longer row is alone anyway
    "E_1_one_row_per_piece": ((4, 1, 0, [1, 2, 1, 3, 1]), [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]),
    # 2 + 2 <= 5 < 2 + 2 + 9; the row of 9 alone; the rest
    "long_row_between_short_rows": ((4, 5, 0, [2, 2, 9, 1, 1]), [(0, 2), (2, 3), (3, 5)]),
    # offsets 0 0 0 2 2 2 2 4 5 5 5: from 0 the last offset <= 3 is off[6] = 2 (off[7] = 4); from 6: 4, 5, 5, 5 less 2 are <= 3
    "empty_runs_before_between_after": ((8, 3, 0, [0, 0, 2, 0, 0, 0, 2, 1, 0, 0]), [(0, 6), (6, 10)]),
    # offsets 0 0 0 5 5 5: the two empty rows in front cannot take the row of 5 along (a piece of no entries), nor can it
    # take anything (alone, beyond E), the empty rows behind it are the last piece (no entries again)
    "empty_pieces_around_a_long_row": ((8, 3, 0, [0, 0, 5, 0, 0]), [(0, 2), (2, 3), (3, 5)]),
    "exactly_E_and_E_plus_1": ((8, 6, 0, [1, 2, 3, 4, 2, 1]), [(0, 3), (3, 5), (5, 6)]),
    # E would allow all ten rows: the chunk limit cuts
    "chunk_limit_cuts": ((4, 100, 0, [1] * 10), [(0, 4), (4, 8), (8, 10)]),
    "rows_left_equal_chunk": ((4, 100, 0, [1] * 8), [(0, 4), (4, 8)]),           # n - a == chunk at a = 0 and at a = 4
    "rows_left_equal_chunk_minus_1": ((4, 100, 0, [1] * 7), [(0, 4), (4, 7)]),   # n - a == chunk - 1 at a = 4
    "n_equal_chunk": ((4, 100, 0, [1, 1, 1, 1]), [(0, 4)]),
    "n_equal_chunk_minus_1": ((4, 100, 0, [1, 1, 1]), [(0, 3)]),
    "one_row_within_E": ((4, 3, 0, [2]), [(0, 1)]),
    "one_row_beyond_E": ((4, 3, 0, [5]), [(0, 1)]),
    "one_empty_row": ((4, 3, 0, [0]), [(0, 1)]),
    "all_rows_empty": ((4, 1, 0, [0] * 9), [(0, 4), (4, 8), (8, 9)]),
    # offsets from 2^40, two rows of 2^39 entries: nothing exceeds E, off[a] + E stays below 2^64; the chunk limit cuts
    "largest_E_offsets_near_2_40": ((4, E_MAX, 2 ** 40, [2 ** 39, 1, 0, 7, 2 ** 39, 3]), [(0, 4), (4, 6)]),
    "largest_E_library_chunk": ((1 << 18, E_MAX, 2 ** 40, [2 ** 39, 1, 0, 7, 2 ** 39, 3]), [(0, 6)]),
    # E = 2^39 at those offsets: the first row is exactly E (and takes nothing: 2^39 + 1 > E), 1 + 0 + 7 fit, the second
    # row of 2^39 is exactly E again, the last row follows alone
    "E_2_39_offsets_near_2_40": ((4, 2 ** 39, 2 ** 40, [2 ** 39, 1, 0, 7, 2 ** 39, 3]), [(0, 1), (1, 4), (4, 5), (5, 6)]),
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the program, built under both sanitizers: a machine without their runtime fails here, it is never run unchecked"""
    out = str(tmp_path_factory.mktemp("pieces") / "csr_pieces")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "csr_pieces.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_the_header_compiles_alone_with_plain_gxx(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(ROOT, "petal-neighbors_amd", "csrc", "csr_pieces.h"))
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_pieces_equal_the_hand_derived_table(exe):
    names = sorted(CASES)
    lines = []
    for name in names:
        chunk, E, base, lens = CASES[name][0]
        off = [base]
        for c in lens:
            off.append(off[-1] + c)
        lines.append(" ".join(str(v) for v in [chunk, E, len(lens)] + off))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(names)
    wrong = []
    for line, name in zip(got, names):
        want = " ".join("%d:%d" % p for p in CASES[name][1])
        if line != want:
            wrong.append((name, line, want))
    assert not wrong, wrong


def test_the_table_covers_every_row_once():
    """(of the table itself: the pieces of a case tile [0, n) in order, none empty of rows)"""
    for name, ((chunk, E, base, lens), pieces) in CASES.items():
        assert pieces[0][0] == 0 and pieces[-1][1] == len(lens), name
        assert all(a < b <= a + chunk for a, b in pieces), name
        assert all(p[1] == q[0] for p, q in zip(pieces, pieces[1:])), name
