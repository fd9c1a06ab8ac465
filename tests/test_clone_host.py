"""The window-clone rule (gc_env.h rep_clone_hdr / rep_clone_table -- what k_clone_boards applies
per table entry) on the host build: a source window built through rep_commit is cloned into a
destination table that holds live and dead entries of other games, under destination generations
below, equal to and above the source's; afterwards both tables answer every rep_commit alike and
nothing the destination held before is live."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "core_host"))
import clonehost as CH  # noqa: E402

# (source generation, destination generation before the clone)
GENS = [(9, 4), (9, 8), (9, 9), (9, 10), (9, 40), (1000, 5), (5, 1000), (0xFFFFFF00, 7)]


@pytest.mark.parametrize("pool,plies,more", [(150, 400, 200), (300, 600, 120), (1, 5, 30), (2, 1, 30)])
@pytest.mark.parametrize("src_gen,dst_gen", GENS)
def test_clone_then_continue(src_gen, dst_gen, pool, plies, more):
    out = np.full(9, -7, dtype=np.int64)
    rc = CH.lib().ch_scenario(1234 + pool, pool, plies, more, src_gen, dst_gen, out.ctypes.data)
    assert rc == 0, rc
    copied, hl, resurrected, first_diff, live_after, max_count, live_before, dead_before, gen_after = out.tolist()
    assert live_before >= 50 and dead_before >= 100  # the destination was dirty, both ways
    assert 1 <= hl <= pool and copied == hl and live_after == hl
    assert gen_after == dst_gen + 1  # bumped once
    assert resurrected == 0
    assert first_diff == -1, f"counts differ from step {first_diff} on"
    if plies >= 400:
        assert hl > 100 and max_count >= 3  # revisits, and a table loaded enough for probe chains


def test_entry_rule_leaves_tag_and_count():
    """rep_clone_table's header: generation replaced, the 32 bits above it unchanged -- seen
    through the scenario's slot-by-slot comparison (out[2]) with a one-board window, whose only
    entry carries count 5"""
    out = np.zeros(9, dtype=np.int64)
    assert CH.lib().ch_scenario(7, 1, 5, 3, 3, 4, out.ctypes.data) == 0
    assert out[0] == 1 and out[2] == 0 and out[3] == -1 and out[5] >= 6
