"""Where the paired kernel's two-tile schedule (Bf16Kernel::PairTwo) is taken, asked on the CPU: tests/cpp/
bf16_choice_meet.cpp includes csrc/bf16_launch.h alone, is compiled with g++ -std=c++17 -Wall -Werror under
AddressSanitizer + UndefinedBehaviorSanitizer and prints bf16_main_kernel's answer for the cases below.

The policy, written down by hand from DESIGN.md 4.10.2 (never by running the function):
  pair applies  = thresholds given (Seeded), aligned grid, 64 slots, no refreshers, q_tiles >= 2
  forced 32     : PairTwo wherever the pair applies, else the 4-wave kernel
  forced 16     : Pair wherever it applies -- never PairTwo
  forced 4 / 8  : as before
  forced 0      : where the paired kernel was chosen before (grid fills the workgroup slots, run_tiles >= 200, image
                  <= 768 MiB): PairTwo if run_tiles >= MIN_RUN_TWO and image <= C2_IMG, else Pair; everything else
                  keeps its kernel
Only the regime measured: MIN_RUN_TWO = 312 are the shortest runs measured in favour of the two-tile schedule (a
500 k-row shard of C2; C2 itself and c5s run 625-tile runs), C2_IMG (15 625 tiles of 17 408 B) the largest image."""
import os
import subprocess

import pytest

from conftest import ROOT

MIB = 1 << 20
IMG = 100 * MIB
TILE = 64 * (2 * 8 + 1) * 16
SCOUT, SELF, SEEDED, RADIUS = 0, 1, 2, 3
F, E, P, P2 = "Four", "Eight", "Pair", "PairTwo"
MIN_RUN_TWO = 312
C2_IMG = 15625 * TILE


def _rows(run, ranges=4):
    return run * ranges * 64


# name: (n, nq_pad, n_wg, split, cap, pass, refreshers, image_bytes, wg_slots), run_tiles,
#       kernel at PN_OPT_BF16_WAVES = (0, 4, 8, 16, 32)
CASES = {
    # the shapes that get the two-tile kernel: 64-slot buffers, two query tiles x 4 ranges on 8 workgroup slots
    "run_312": ((_rows(MIN_RUN_TWO), 512, 8, 1, 64, SEEDED, 0, IMG, 8), 312, (P2, F, E, P, P2)),
    "run_600": ((_rows(600), 512, 8, 1, 64, SEEDED, 0, IMG, 8), 600, (P2, F, E, P, P2)),
    "run_625_c2": ((1_000_000, 10240, 1000, 1, 64, SEEDED, 0, 15625 * TILE, 512), 625, (P2, F, E, P, P2)),
    "run_2000_at_c2_image": ((_rows(2000), 512, 8, 1, 64, SEEDED, 0, C2_IMG, 8), 2000, (P2, F, E, P, P2)),
    "run_600_three_query_tiles": ((_rows(600), 768, 12, 1, 64, SEEDED, 0, IMG, 12), 600, (P2, F, E, P, P2)),
    "run_312_c2s2": ((500_000, 10240, 1000, 1, 64, SEEDED, 0, 7813 * TILE, 512), 312, (P2, F, E, P, P2)),
    # the shapes that keep the paired kernel: runs from 200 tiles up to the two-tile kernel's shortest, larger images
    "run_311": ((_rows(311), 512, 8, 1, 64, SEEDED, 0, IMG, 8), 311, (P, F, E, P, P2)),
    "run_2000_one_tile_above_c2_image": ((_rows(2000), 512, 8, 1, 64, SEEDED, 0, C2_IMG + TILE, 8), 2000, (P, F, E, P, P2)),
    "run_2000_at_768MiB": ((_rows(2000), 512, 8, 1, 64, SEEDED, 0, 768 * MIB, 8), 2000, (P, F, E, P, P2)),
    "run_200": ((_rows(200), 512, 8, 1, 64, SEEDED, 0, IMG, 8), 200, (P, F, E, P, P2)),
    # the shapes that keep the 4-wave kernel (the two-tile kernel could run: only a forced 32 takes it)
    "run_600_grid_does_not_fill": ((_rows(600, 3), 512, 6, 1, 64, SEEDED, 0, IMG, 8), 600, (F, F, E, P, P2)),
    "run_600_slots_unknown": ((_rows(600), 512, 8, 1, 64, SEEDED, 0, IMG, 0), 600, (F, F, E, P, P2)),
    "run_600_above_768MiB": ((_rows(600), 512, 8, 1, 64, SEEDED, 0, 768 * MIB + TILE, 8), 600, (F, F, E, P, P2)),
    # ... and where no paired kernel applies, forced or not
    "run_600_one_query_tile": ((_rows(600, 8), 256, 8, 1, 64, SEEDED, 0, IMG, 8), 600, (F, F, E, F, F)),
    "run_600_refreshers": ((_rows(600), 512, 8, 1, 64, SEEDED, 1, IMG, 8), 600, (F, F, E, F, F)),
    "run_600_slots_128": ((_rows(600), 512, 8, 1, 128, SEEDED, 0, IMG, 8), 600, (E, F, E, F, F)),
    "run_600_self_scout": ((_rows(600), 512, 8, 1, 64, SELF, 0, IMG, 8), 600, (F, F, F, F, F)),
    "run_600_radius": ((_rows(600), 512, 8, 1, 256, RADIUS, 0, IMG, 8), 600, (F, F, F, F, F)),
    "unaligned_split_2": ((_rows(600), 512, 8, 2, 64, SEEDED, 0, IMG, 8), 0, (F, F, F, F, F)),
    # short runs: the 8-wave kernel by the rule, the two-tile kernel only when forced
    "run_199": ((_rows(199), 512, 8, 1, 64, SEEDED, 0, IMG, 8), 199, (E, F, E, P, P2)),
    "run_16": ((_rows(16), 512, 8, 1, 64, SEEDED, 0, IMG, 8), 16, (E, F, E, P, P2)),
}
WAVES = (0, 4, 8, 16, 32)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("choice_meet") / "bf16_choice_meet")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "bf16_choice_meet.cpp"), "-o", out]
    san = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        r = subprocess.run(base, capture_output=True, text=True)  # no sanitizer runtime here: the table is still checked
    assert r.returncode == 0, r.stderr
    return out


def test_policy_table(exe):
    names = sorted(CASES)
    lines = [" ".join(str(v) for v in CASES[name][0] + (w,)) for name in names for w in WAVES]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    wrong = []
    for i, name in enumerate(names):
        _, run, kernels = CASES[name]
        for j, w in enumerate(WAVES):
            want = "%s 1 %d" % (kernels[j], run)  # (whatever is chosen must be able to run: "applies" is 1)
            if got[len(WAVES) * i + j] != want:
                wrong.append((name, w, got[len(WAVES) * i + j], want))
    assert not wrong, wrong
