"""The split-K planner of the weight-gradient launchers (csrc/wgrad_launch.h: plan_split_k, plan_split_k_doubling, reached through
pfst_wgrad_split_k -- host arithmetic, no GPU) against tests/golden/wgrad_split_k.txt.  The table was written by a program holding the C++
loops of the commit named in its first line verbatim -- the five copies of the efficiency loop the launchers had then (they differed in
`slots` and the K-step only), conv_mfma's gridDim.z clamp and the doubling loop of the generic bf16x6 kernel -- so a row that fails here
means a launcher no longer cuts its pixel range as it did then.  Retuning the rule (its constants are in one place now) means regenerating
the table on purpose.

Rows: `work P slots k_step chunk_cap doubling chunks chunk_len tags`.  The clamp rows come in two kinds.  Tag c: conv_mfma's launcher as it
calls the planner, chunk_cap = 65535 / N and work = tiles * N; there the clamp cannot bind (N > 1023 is at least one round of workgroups
before any split, and the loop stops near 14 rounds: N * chunks stays below ~14 400).  Tag C: the same statements with the loop fed few
workgroups and the clamp many images, where it does bind -- a combination only the host entry point can be given."""
import os

import pytest

from pfst_amd import hip_ops as ops

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad_split_k.txt')
PAIRS = {(256, 16), (512, 16), (768, 16), (1024, 16), (512, 32)}        # every (slots, K-step) a launcher passes
TAGS = {'r': 'rounds < 2 at the chosen split', 'e': 'the >= 0.93 early exit', 'p': 'the P / c >= 512 stop', 'm': 'the c == 64 stop',
        'g': 'a ragged last chunk', 's': 'chunks shrinking in the final cdiv', 'c': 'the clamp as conv_mfma reaches it',
        'C': 'the clamp binding (N above 1023)', 'd': 'the doubling rule'}


@pytest.fixture(scope='module')
def rows():
    lines = open(TABLE).read().splitlines()
    assert lines[0].startswith('# split-K plans recorded from the C++ text of commit ')
    out = []
    for ln in lines:
        if not ln.startswith('#'):
            f = ln.split()
            out.append((tuple(int(v) for v in f[:8]), f[8]))
    return out


def test_table_covers_every_case(rows):
    assert {(r[2], r[3]) for r, t in rows if 'd' not in t} == PAIRS
    for tag, what in TAGS.items():
        hit = [r for r, t in rows if tag in t]
        assert hit, f'no row for {what}'
        for pair in PAIRS if tag in 'repmgs' else ():
            assert any((r[2], r[3]) == pair for r in hit if not r[5]), f'no row for {what} at slots, K-step = {pair}'
    assert all(r[4] < 64 and r[6] <= r[4] for r, t in rows if 'C' in t), 'a binding clamp row: N above 1023, chunks within the cap'
    assert any('s' in t for r, t in rows if r[5]) and any('g' in t for r, t in rows if r[5]), 'the doubling rule: ragged and shrinking rows'
    # not a table of trivial rows: at least a third split the pixel range at all
    split = sum(1 for r, _ in rows if r[6] > 1)
    assert 3 * split >= len(rows), f'{split} of {len(rows)} rows have more than one chunk'


def test_library_planner_matches_the_recorded_table(rows):
    bad = []
    for (work, P, slots, k_step, cap, doubling, chunks, chunk_len), tags in rows:
        got = ops.wgrad_split_k(work, P, slots, k_step, cap, doubling)
        if got != (chunks, chunk_len):
            bad.append(((work, P, slots, k_step, cap, doubling), tags, (chunks, chunk_len), got))
    assert not bad, f'{len(bad)} of {len(rows)} rows differ; first (arguments, tags, recorded, library): {bad[:5]}'


def test_plans_cover_the_pixels_in_whole_steps(rows):
    """what every kernel relies on: chunks * chunk_len covers P, no chunk is empty, chunk_len is a whole number of K-steps"""
    for (work, P, slots, k_step, cap, doubling, _, _), _ in rows:
        chunks, chunk_len = ops.wgrad_split_k(work, P, slots, k_step, cap, doubling)
        step, most = (16, 1024) if doubling else (k_step, 64)        # doubling stops at 1024 workgroups: at most 1024 chunks
        assert 1 <= chunks <= most and chunk_len % step == 0 and (chunks - 1) * chunk_len < P <= chunks * chunk_len, (work, P, slots, k_step, cap)
        assert not cap or chunks <= cap


def test_planner_refuses_bad_arguments():
    from pfst_amd._lib import PfstHipError
    for args in ((0, 1024, 1024, 16), (4, 0, 1024, 16), (4, 1024, 0, 16), (4, 1024, 1024, 0), (4, 1024, 1024, 16, -1)):
        with pytest.raises(PfstHipError, match='pfst_wgrad_split_k failed \\(-1\\)'):
            ops.wgrad_split_k(*args)
    assert ops.wgrad_split_k(4, 5120, doubling=True) == (8, 640)          # slots and K-step are not read by the doubling rule
