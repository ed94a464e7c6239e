"""CPU test (no GPU) of the one statement of "has this arrival counter reached its target" behind the chained launches' waits:
csrc/common.h chain_reached, compiled into a host program.

The update's chained forward and backward launches hand data between workgroups of ONE launch through `unsigned` arrival counters
that are never reset.  Between updates a counter holds epoch x T (T = its arrivals per update); a consumer of update number e waits
for (epoch word + epoch_bias) x T = (e + 1) x T arrivals -- the forward chain reads the epoch word before the update's head kernel
has bumped it (bias 1), the backward chain after (bias 0).  Counter and product both wrap modulo 2^32, so the comparison has to be
by modular distance; `count < target` lets every consumer through, unwaited, in the update whose target first passes 2^32 (at
2^32 / 288 = 14.9 M updates for conv3's weight-gradient counter at batch 32).

The table below restates by hand every arrival count the launches use (tests/test_gpu_chain_counter_wrap.py holds it against what
the library reports); 2, 64 and 128 are the power-of-two cases, whose target wraps to exactly 0."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# arrivals per update on one counter, by class (NatureConvBody, 256-thread workgroups of 32 positions x 32 channels)
ARRIVALS = {
    "fwd_conv1_to_conv2": [13],          # conv1: 400 positions = 13 tiles of 32, 32 channels = 1 group
    "fwd_conv2_to_conv3": [6],           # conv2: 81 positions = 3 tiles, 64 channels = 2 groups
    "bwd_conv3_dgrad": [6],              # stride 1: 1 phase x 3 tiles of its input's 81 positions x 2 input-channel groups
    "bwd_conv2_dgrad": [8],              # stride 2: 4 phases x 2 pairs of the 4 tiles of 100 input positions x 1 input-channel group
    "bwd_conv3_wgrad": [153, 288],       # 9 k-groups x batch (17, 32): one counter for all samples
    "bwd_conv2_wgrad": [68, 128],        # 4 k-groups x batch
    "bwd_fc4_dgrad": [98],               # 3136 / 32 column tiles (DRA_VAR_BWD_CHAIN_FC)
}
POWERS_OF_TWO = [2, 64, 128]
ALL_T = sorted({t for v in ARRIVALS.values() for t in v} | set(POWERS_OF_TWO))

PROBE = r'''
#include "deeprl_amd/csrc/common.h"
#include <stdio.h>
#include <stdlib.h>
// the parent's expression: the wait went on while (count < target)
static bool old_reached(unsigned count, unsigned target) { return !(count < target); }
int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const unsigned long long T = strtoull(argv[i], nullptr, 10);
    const unsigned long long wrap = ((1ull << 32) + T - 1) / T;            // first update count whose product reaches 2^32
    unsigned long long epochs[16]; int near[16]; int ne = 0;
    for (long long d = -3; d <= 3; ++d) { epochs[ne] = wrap + d; near[ne++] = 1; }
    const unsigned long long far[3] = {0ull, 1ull, (1ull << 31) / T};
    for (int k = 0; k < 3; ++k) { epochs[ne] = far[k]; near[ne++] = 0; }
    unsigned long long checked = 0, new_wrong = 0, old_wrong_near = 0, old_wrong_far = 0;
    for (int k = 0; k < ne; ++k)
      for (unsigned bias = 0; bias <= 1; ++bias)
        for (unsigned long long a = 0; a <= T; ++a) {
          const unsigned long long e = epochs[k];                          // updates completed before this one
          const unsigned count = (unsigned)(e * T + a);                    // the counter after `a` arrivals of this update
          const unsigned epoch_word = (unsigned)(e + 1ull - bias);         // (bias 0: this update's head kernel has bumped it)
          const unsigned target = (epoch_word + bias) * (unsigned)T;       // mega_wait's product, 32-bit unsigned
          const bool want = a == T;
          ++checked;
          if (chain_reached(count, target) != want) {
            if (++new_wrong <= 4) printf("# chain_reached wrong: T %llu e %llu bias %u a %llu count %u target %u\n", T, e, bias, a, count, target);
          }
          if (old_reached(count, target) != want) { if (near[k]) ++old_wrong_near; else ++old_wrong_far; }
        }
    printf("%llu %llu %llu %llu %llu %llu\n", T, wrap, checked, new_wrong, old_wrong_near, old_wrong_far);
  }
  return 0;
}
'''


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("needs hipcc")
    d = tmp_path_factory.mktemp("chain_wrap")
    src = d / "probe.cpp"
    src.write_text(PROBE)
    exe = str(d / "probe")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-I", ROOT, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                   check=True, capture_output=True)
    out = subprocess.run([exe] + [str(t) for t in ALL_T], check=True, capture_output=True, text=True).stdout
    print(out)
    got = {}
    for line in out.splitlines():
        if not line.startswith("#"):
            f = [int(x) for x in line.split()]
            got[f[0]] = dict(wrap=f[1], checked=f[2], new_wrong=f[3], old_wrong_near=f[4], old_wrong_far=f[5])
    return got


def test_every_arrival_count_and_the_powers_of_two_are_probed(rows):
    assert sorted(rows) == ALL_T and {2, 64, 128, 288, 153, 68, 98, 13, 6, 8} <= set(rows)
    for t, r in rows.items():
        assert r["wrap"] == -(-(1 << 32) // t)
        assert r["checked"] == (7 + 3) * 2 * (t + 1)      # epochs x both biases x arrival numbers 0 .. T


@pytest.mark.parametrize("t", ALL_T)
def test_chain_reached_is_true_exactly_when_the_arrivals_are_complete(rows, t):
    """+-3 updates around the wrap ceil(2^32 / T) and far from it (updates 0, 1 and 2^31 / T), both epoch biases, every arrival
    number 0 .. T: reached exactly at T arrivals, never before."""
    assert rows[t]["new_wrong"] == 0


@pytest.mark.parametrize("t", ALL_T)
def test_the_plain_comparison_fails_at_the_wrap_and_only_there(rows, t):
    """The negative control: the parent's `count < target` gives a wrong answer in the wrap window for every arrival count (this
    test would have caught it), and none far from the wrap (why no existing test did)."""
    assert rows[t]["old_wrong_near"] >= 1
    assert rows[t]["old_wrong_far"] == 0


def test_the_predicate_agrees_with_exact_integer_arithmetic():
    """The same statement in Python's unbounded integers, against the true counts (no 32-bit arithmetic on the reference side): for
    every T of the table, every update in the window and every arrival number, modular distance < 2^31 <=> arrivals >= needed."""
    M = 1 << 32
    for t in ALL_T:
        wrap = -(-M // t)
        for e in list(range(wrap - 3, wrap + 4)) + [0, 1, (1 << 31) // t]:
            need = (e + 1) * t
            for a in range(t + 1):
                have = e * t + a
                assert (((have % M) - (need % M)) % M < (1 << 31)) == (have >= need), (t, e, a)
