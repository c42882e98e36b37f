"""What test_gpu_replay_tail.py's inputs make the replay kernel do, shown on the census model alone
(tools/replay_census.py: the chunk schedule of replay_shuffle_t in plain Python, checked against random.shuffle):
every kind of tail chunk listed below occurs at least once among the levels, MT indices and debts used there."""
import random

import pytest

from replay_tail_cases import B, LEVELS, TAIL, cpython, env_case  # (puts tools/ on the path)
import replay_census as RC


@pytest.fixture(scope='module')
def chunks():
    """Every chunk of every env of every level (the full-temper run repeats large8's schedule: skipped)."""
    out = []
    for level, (cfg, variant, nf) in enumerate(LEVELS):
        if variant:
            continue
        for e in range(B):
            mt, mti, debt = env_case(level, e)
            perm = list(range(nf))
            cs, idx = RC.simulate(cpython(mt, mti), nf - 1, debt, idx0=mti, tail=TAIL, perm=perm)
            r = cpython(mt, mti)
            want = list(range(nf))
            for _ in range(debt):
                r.shuffle(want)
            assert perm == want and idx == r.getstate()[1][624], (cfg, e)
            for c in cs:
                c.update(level=cfg, env=e, debt=debt)
            out += cs
    return out


def test_census_reproduces_the_measured_schedule():
    """29.7 chunks per shuffle (PMC: 134.3M chunks / 65,536 envs / 69 shuffles) and 1.91 Jacobi rounds per chunk at
    nf = 1077 with one width per chunk; with the tail at 95, 25.8 chunks, 2.1 of them mixed; at 127, 25.8 and 3.1."""
    c = RC.census(1077, shuffles=300)
    assert abs(c['chunks_per_shuffle'] - 29.7) < 0.15
    assert abs(c['jacobi_rounds_per_chunk'] - 1.91) < 0.03
    t = RC.census(1077, shuffles=300, tail=TAIL)
    assert abs(t['chunks_per_shuffle'] - 25.8) < 0.15 and abs(t['tail_chunks_per_shuffle'] - 2.1) < 0.15
    t = RC.census(1077, shuffles=300, tail=127)
    assert abs(t['chunks_per_shuffle'] - 25.7) < 0.15 and abs(t['tail_chunks_per_shuffle'] - 3.04) < 0.15
    u = RC.census(1077, shuffles=300, tail=0)
    assert u['tail_chunks_per_shuffle'] == 0


def test_tail_chunk_crosses_the_state_end(chunks):
    assert any(c['mixed'] and c['crosses'] and not c['twist'] for c in chunks)


def test_tail_chunk_starts_past_the_state_end(chunks):
    """idx >= 624 when the chunk begins: the state is regenerated first."""
    assert any(c['mixed'] and c['twist'] for c in chunks)


def test_tail_chunk_leaves_words_to_the_next_shuffle(chunks):
    hit = [c for c in chunks if c['mixed'] and c['ends'] and c['consumed'] < 64 and c['shuffle'] + 1 < c['debt']]
    assert hit
    assert any(c['idx'] + c['consumed'] > 624 for c in hit)  # also with the leftover words in the next state


def test_tail_chunk_without_an_accepted_lane_does_not_exist(chunks):
    """While nothing is accepted every lane of a tail chunk draws at i = icur >= 1 and rejects with probability
    1 - (i + 1) / 2^bitlen(i + 1) <= 1/2 (1/2 where i + 1 is a power of two): a chunk without an accepted lane has
    probability <= 2^-64. None occurs in the cases, and none among the first chunks of 10^4 seeds at i = 63, the
    most favourable rank. (The kernel runs such a chunk's swap block on the sinks, as the main loop does.)"""
    assert not any(c['mixed'] and c['nacc'] == 0 for c in chunks)
    for seed in range(10000):
        r = random.Random(seed)
        n = 0
        while n < 64 and (r.getrandbits(32) >> 25) > 63:
            n += 1
        assert n < 64, seed


def test_tail_jacobi_of_six_rounds(chunks):
    assert max(c['rounds'] for c in chunks if c['mixed']) >= 6


def test_tail_chunks_on_both_forward_paths(chunks):
    paths = {c['path'] for c in chunks if c['mixed']}
    assert {'none', 'serial', 'table'} <= paths


def test_shuffle_starts_inside_the_tail(chunks):
    assert any(c['mixed'] and c['starts'] and c['shuffle'] > 0 for c in chunks)
    assert any(not c['mixed'] and c['starts'] for c in chunks)  # and the main loop runs where hi > TAIL
    assert any(c['mixed'] and not c['starts'] and c['icur'] <= TAIL for c in chunks if c['level'] == 'large8.yaml')
