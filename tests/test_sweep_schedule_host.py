"""The backward sweep's ring schedule (csrc/sweep_schedule.h: batch_slot) as a table.  Host only: a stand-alone program that includes nothing but that header is
compiled for the host, prints `batch slot flush` for every timestep, and is compared with a restatement of the lambda the sweep carried before the schedule
became a function -- which also has to satisfy what the sweep relies on."""
import os
import subprocess

import pytest

from pivp_amd import _lib

CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), 'csrc')
TS = range(2, 21)      # sequence lengths
GS = range(1, 9)       # timesteps per launch: 1 .. WG_BATCH_MAX (the rings use min(T - 2, 8), cut to the mode's or the option's choice)

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "sweep_schedule.h"
int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const int t_lo = atoi(argv[1]), t_hi = atoi(argv[2]), g_lo = atoi(argv[3]), g_hi = atoi(argv[4]);
    for (int T = t_lo; T <= t_hi; ++T)
        for (int G = g_lo; G <= g_hi; ++G)
            for (int t = T - 2; t >= 0; --t) {
                const pivp::BatchSlot b = pivp::batch_slot(T, t, G);
                printf("%d %d %d %d %d %d\n", T, G, t, b.batch, b.slot, b.flush ? 1 : 0);
            }
    return 0;
}
'''


def sched(T, t, G):
    """-> (batch, slot, flush): the `sched` lambda of rollout_backward_sweep as it stood before csrc/sweep_schedule.h, line by line"""
    k, n = T - 2 - t, T - 2
    tail = 2 if (G > 2 and n > 2) else 0
    body = n - tail
    nb_body = (body + G - 1) // G
    if t == 0:
        return nb_body + (1 if tail else 0), 0, True
    if k < body:
        slot = k % G
        return k // G, slot, slot == G - 1 or k == body - 1
    return nb_body, k - body, k == n - 1


@pytest.fixture(scope='module')
def expected():
    return {(T, G): [sched(T, t, G) for t in range(T - 2, -1, -1)] for T in TS for G in GS}


@pytest.fixture(scope='module')
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp('sweep_schedule')
    src, exe = str(d / 'schedule.cpp'), str(d / 'schedule')
    with open(src, 'w') as f:
        f.write(PROGRAM)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')      # the compiler build.py uses; host only: plain C++, no device code, no library
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, src, '-o', exe])
    out = subprocess.check_output([exe, str(TS[0]), str(TS[-1]), str(GS[0]), str(GS[-1])]).decode()
    table = {}
    for line in out.splitlines():
        T, G, t, b, slot, flush = (int(x) for x in line.split())
        table.setdefault((T, G), []).append((t, b, slot, bool(flush)))
    return table


def test_the_header_computes_what_the_sweep_computed(built, expected):
    assert sorted(built) == sorted(expected)
    for key, rows in expected.items():
        T = key[0]
        assert [r[0] for r in built[key]] == list(range(T - 2, -1, -1)), key
        assert [r[1:] for r in built[key]] == rows, key


def test_the_schedule_keeps_what_the_sweep_relies_on(expected):
    for (T, G), rows in expected.items():
        steps = list(range(T - 2, -1, -1))
        batches = []      # [(batch, [(t, slot, flush), ...])] in sweep order
        for t, (b, slot, flush) in zip(steps, rows):
            if not batches or batches[-1][0] != b:
                batches.append((b, []))
            batches[-1][1].append((t, slot, flush))
        where = 'T = %d, G = %d' % (T, G)
        # consecutive batches alternate ring parity: the batch numbers count up by one
        assert [b for b, _ in batches] == list(range(len(batches))), where
        for b, members in batches:
            # slots 0 .. k without gaps, only the batch's last step flushes, no batch longer than G
            assert [m[1] for m in members] == list(range(len(members))), where
            assert [m[2] for m in members] == [False] * (len(members) - 1) + [True], where
            assert len(members) <= G, where
        # t = 0 (no h input) is alone in the last batch and flushes
        assert batches[-1][1] == [(0, 0, True)], where
        # deep batches: the last two batched timesteps form a batch of their own
        if G > 2 and T - 2 > 2:
            assert [m[0] for m in batches[-2][1]] == [2, 1], where
