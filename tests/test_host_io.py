"""Where the slots of a host entry point's staging buffer lie, asked on the CPU: tests/cpp/host_io.cpp includes
csrc/host_io.h alone (host arithmetic, no HIP), is compiled with g++ -std=c++17 -Wall -Werror under AddressSanitizer +
UndefinedBehaviorSanitizer, and prints the offsets and the total of the slots it is given.

The expected numbers were worked out BY HAND from the rule, never by running the header.  A call declares slots in
order, each an element size and a count:
  off[0] = 0,  off[i] = the end of slot i - 1 rounded up to a multiple of 16,  end = off + size * count,
  total  = the end of the last slot;
a count of 0 is a slot of no bytes; at most 8 slots; a product or a sum that does not fit 64 bits is an error.
Worked through for "every_boundary_padded" (sizes 8 4 1 8, counts 3 5 7 3): 0 .. 24; 24 -> 32, 32 + 20 = 52; 52 -> 64,
64 + 7 = 71; 71 -> 80, 80 + 24 = 104."""
import os
import subprocess

import pytest

from conftest import ROOT

ERROR = "error"

# name: [(element size, count), ...], (offsets, total) or ERROR
CASES = {
    "single_slot": ([(4, 5)], ([0], 20)),
    "every_boundary_padded": ([(8, 3), (4, 5), (1, 7), (8, 3)], ([0, 32, 64, 80], 104)),
    # 4 * 4 = 16, 16 + 8 * 2 = 32, 32 + 16 = 48: every slot ends on a multiple of 16
    "no_padding_needed": ([(4, 4), (8, 2), (1, 16)], ([0, 16, 32], 48)),
    # 0 .. 0; 0 .. 12; 12 -> 16 .. 16; 16 .. 21; 21 -> 32 .. 32 (an empty last slot still starts on its boundary)
    "zero_counts_first_middle_last": ([(8, 0), (4, 3), (8, 0), (1, 5), (4, 0)], ([0, 0, 16, 16, 32], 32)),
    "only_zero_counts": ([(8, 0), (4, 0)], ([0, 0], 0)),
    "slot_bound_reached": ([(1, 1)] * 8, ([0, 16, 32, 48, 64, 80, 96, 112], 113)),
    "slot_bound_passed": ([(1, 1)] * 9, ERROR),
    # 8 * (2^61 - 1) = 2^64 - 8 fits; 8 * 2^61 = 2^64 does not
    "largest_product_that_fits": ([(8, 2 ** 61 - 1)], ([0], 2 ** 64 - 8)),
    "product_overflows": ([(8, 2 ** 61)], ERROR),
    "product_overflows_behind_a_slot": ([(4, 3), (2 ** 33, 2 ** 31)], ERROR),
    # 2^63 + 2^63 = 2^64
    "sum_overflows": ([(1, 2 ** 63), (1, 2 ** 63)], ERROR),
    "sum_fits_exactly": ([(1, 2 ** 63), (1, 2 ** 63 - 1)], ([0, 2 ** 63], 2 ** 64 - 1)),
    # the slot ends at 2^64 - 1: the next boundary is 2^64
    "padding_overflows": ([(1, 2 ** 64 - 1), (1, 1)], ERROR),
}

# The two largest layouts of csrc/index.hip, slot by slot as km_host and ms_host declare them, for T = float (4 bytes)
# and double (8): name -> (slots, (offsets, total), the byte count the hand-written sum before HostIo asked for).
N, NC, DIM, NS, N_H = 777, 3, 5, 51, 1


def km_slots(t):  # centres T [nc][dim] | labels i64 [n] | dist T [n] | counts u64 [nc] | inertia f64 | iterations u64 | shift2 f64
    return [(t, NC * DIM), (8, N), (t, N), (8, NC), (8, 1), (8, 1), (8, 1)]


def ms_slots(t):  # h T [n_h] | modes T [ns][dim] | points u64 [ns] | iterations u32 [ns] | shift f64 [ns]
    return [(t, N_H), (t, NS * DIM), (8, NS), (4, NS), (8, NS)]


def up8(v):
    return (v + 7) // 8 * 8


ENTRY_LAYOUTS = {
    # 60; 64 + 6216 = 6280; 6288 + 3108 = 9396; 9408 + 24 = 9432; 9440 + 8; 9456 + 8; 9472 + 8 = 9480
    "km_host_f32": (km_slots(4), ([0, 64, 6288, 9408, 9440, 9456, 9472], 9480),
                    N * 8 + 24 + NC * 8 + up8(N * 4) + up8(NC * DIM * 4)),
    # 120; 128 + 6216 = 6344; 6352 + 6216 = 12568; 12576 + 24 = 12600; 12608 + 8; 12624 + 8; 12640 + 8 = 12648
    "km_host_f64": (km_slots(8), ([0, 128, 6352, 12576, 12608, 12624, 12640], 12648),
                    N * 8 + 24 + NC * 8 + up8(N * 8) + up8(NC * DIM * 8)),
    # 4; 16 + 1020 = 1036; 1040 + 408 = 1448; 1456 + 204 = 1660; 1664 + 408 = 2072
    "ms_host_f32": (ms_slots(4), ([0, 16, 1040, 1456, 1664], 2072),
                    NS * (8 + 8 + 4) + up8(NS * DIM * 4) + up8(N_H * 4)),
    # 8; 16 + 2040 = 2056; 2064 + 408 = 2472; 2480 + 204 = 2684; 2688 + 408 = 3096
    "ms_host_f64": (ms_slots(8), ([0, 16, 2064, 2480, 2688], 3096),
                    NS * (8 + 8 + 4) + up8(NS * DIM * 8) + up8(N_H * 8)),
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the program, built under both sanitizers: a machine without their runtime fails here, it is never run unchecked"""
    out = str(tmp_path_factory.mktemp("host_io") / "host_io")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "host_io.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def ask(exe, slot_lists):
    lines = [" ".join(str(v) for v in [len(slots)] + [x for s in slots for x in s]) for slots in slot_lists]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(slot_lists)
    return got


def line_of(want):
    return ERROR if want == ERROR else " ".join(str(v) for v in want[0] + [want[1]])


def test_the_header_compiles_alone_with_plain_gxx(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(ROOT, "petal-neighbors_amd", "csrc", "host_io.h"))
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_layouts_equal_the_hand_derived_table(exe):
    names = sorted(CASES)
    got = ask(exe, [CASES[name][0] for name in names])
    wrong = [(name, line, line_of(CASES[name][1])) for line, name in zip(got, names) if line != line_of(CASES[name][1])]
    assert not wrong, wrong


def test_the_entry_points_largest_layouts(exe):
    names = sorted(ENTRY_LAYOUTS)
    got = ask(exe, [ENTRY_LAYOUTS[name][0] for name in names])
    for line, name in zip(got, names):
        slots, want, hand_sum = ENTRY_LAYOUTS[name]
        assert line == line_of(want), (name, line)
        *off, total = [int(v) for v in line.split()]
        assert all(o % 16 == 0 for o in off), (name, off)
        assert total >= hand_sum, (name, total, hand_sum)


def test_the_tables_follow_the_rule_they_state():
    """(of the tables themselves: slots in order, 16-byte starts, nothing overlaps, the total is the last end)"""
    for name, (slots, want) in list(CASES.items()) + [(k, v[:2]) for k, v in ENTRY_LAYOUTS.items()]:
        if want == ERROR:
            continue
        off, total = want
        assert len(off) == len(slots) <= 8 and off[0] == 0, name
        ends = [o + e * c for o, (e, c) in zip(off, slots)]
        assert all(o % 16 == 0 and 0 <= o - end < 16 for o, end in zip(off[1:], ends)), name
        assert total == ends[-1], name
