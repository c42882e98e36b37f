#!/usr/bin/env python3
"""Chunk census of the replay kernel's shuffle (replay_shuffle_t, csrc/mfg_kernels.h), modelled on the CPU in plain
Python: no GPU, no library. A chunk is 64 MT19937 words. A uniform chunk uses one bit width k = bitlen(icur + 1) and
stops where the width would change; a mixed chunk (the tail, icur <= T) takes each lane's width from its own rank
and stops only where the shuffle ends. For a floor count the census prints chunks per shuffle, how many of them are
tail chunks, Jacobi rounds per chunk, and the forwards per chunk split into the serial (<= RP_SERIAL_FWD) and the
table path. The tempered words come from CPython's own generator (getrandbits(32)), and every shuffle's swaps are
checked against random.shuffle, so the model is exact by construction.
usage: python tools/replay_census.py [--nf 1077] [--tail T] [--all-mixed] [--band-left S] [--seed-kind 34|sure]
       [--shuffles 300]"""
import argparse
import json
import random

WAVE = 64
MT_N = 624
RP_SERIAL_FWD = 4  # csrc/mfg_kernels.h
LO = 1


class Stream:
    """The tempered 32-bit outputs of a CPython generator from its current state on, by absolute position."""

    def __init__(self, rng):
        self.rng, self.w = rng, []

    def get(self, pos, n=WAVE):
        while len(self.w) < pos + n:
            self.w.append(self.rng.getrandbits(32))
        return self.w[pos:pos + n]


def seed34(lane):
    return (3 * lane) >> 2


def seed_sure(lane):
    return lane


def _fixed_point(accept, seed_rank):
    """Jacobi iteration m <- {l : accept(l, #m below l)} from the seed evaluated at rank seed_rank(l). Returns the
    accepted lanes' ranks A (by lane), the stable set and the number of rounds (ballots after the seed's)."""
    m = [accept(l, seed_rank(l)) for l in range(WAVE)]
    rounds = 0
    while True:
        A, a = [], 0
        for l in range(WAVE):
            A.append(a)
            a += m[l]
        m2 = [accept(l, A[l]) for l in range(WAVE)]
        rounds += 1
        if m2 == m:
            return A, m, rounds
        m = m2


def chunk_uniform(y, icur, seed_rank=seed34):
    """One width per chunk. Returns (accepted [(lane, i, j)], consumed, rounds)."""
    k = (icur + 1).bit_length()
    span = icur - max(LO, (1 << (k - 1)) - 1)
    r = [w >> (32 - k) for w in y]
    c = [min(icur - r[l], span) for l in range(WAVE)]
    A, m, rounds = _fixed_point(lambda l, a: a <= c[l], seed_rank)
    acc = [(l, icur - A[l], r[l]) for l in range(WAVE) if m[l]]
    consumed = acc[-1][0] + 1 if len(acc) > span else WAVE
    # the sequential walk (CPython's order) gives the same set
    seq, a = [], 0
    for l in range(WAVE):
        if a > span:
            break
        if r[l] <= icur - a:
            seq.append((l, icur - a, r[l]))
            a += 1
    assert seq == acc, 'the Jacobi fixed point is the sequential walk'
    return acc, consumed, rounds


def chunk_mixed(y, icur, seed_rank=seed34):
    """Per-lane widths: i = icur - A, r = y >> (32 - bitlen(i + 1)), accept <=> i >= LO and r <= i."""
    def draw(l, a):
        i = icur - a
        return y[l] >> (32 - (max(i, 0) + 1).bit_length())

    def accept(l, a):
        i = icur - a
        return i >= LO and draw(l, a) <= i

    A, m, rounds = _fixed_point(accept, seed_rank)
    acc = [(l, icur - A[l], draw(l, A[l])) for l in range(WAVE) if m[l]]
    consumed = acc[-1][0] + 1 if len(acc) == icur - LO + 1 else WAVE
    seq, i = [], icur
    for l in range(WAVE):
        if i < LO:
            break
        r = y[l] >> (32 - (i + 1).bit_length())
        if r <= i:
            seq.append((l, i, r))
            i -= 1
    assert seq == acc, 'the Jacobi fixed point is the sequential walk'
    return acc, consumed, rounds


def simulate(rng, hi, shuffles, idx0=None, tail=0, all_mixed=False, seed_rank=seed34, perm=None, band_left=0):
    """The chunk schedule of `shuffles` shuffles of hi + 1 cells from rng's state (a random.Random; its state is not
    advanced in step: the words are read ahead). idx0: the state's mt index at the start (default: rng's own).
    band_left: chunks that start with fewer than this many ranks left in their width band are mixed too.
    Returns (chunks, final mt index); with a list `perm`, it is shuffled in place (the swaps in order).
    Each chunk: dict(shuffle, icur, idx (the kernel's idx when the chunk's words are read), twist (the state was
    regenerated first), crosses (words past 623 computed from the current state), mixed, nacc, consumed, rounds,
    forwards, path ('none' | 'serial' | 'table'), ends, starts (the shuffle's first chunk))."""
    if idx0 is None:
        idx0 = rng.getstate()[1][-1]
    st = Stream(rng)
    pos, idx, out = 0, idx0, []
    for s in range(shuffles):
        icur = hi
        while icur >= LO:
            mixed = all_mixed or icur <= tail or icur - ((1 << ((icur + 1).bit_length() - 1)) - 1) < band_left
            twist = idx >= MT_N
            if twist:
                idx -= MT_N
            y = st.get(pos)
            acc, consumed, rounds = (chunk_mixed if mixed else chunk_uniform)(y, icur, seed_rank)
            nacc = len(acc)
            inext = icur - nacc
            fwd = sum(1 for _, i, j in acc if inext < j < i)
            if perm is not None:
                for _, i, j in acc:
                    perm[i], perm[j] = perm[j], perm[i]
            out.append(dict(shuffle=s, icur=icur, idx=idx, twist=twist, crosses=idx > MT_N - WAVE, mixed=mixed,
                            nacc=nacc, consumed=consumed, rounds=rounds, forwards=fwd,
                            path='none' if not fwd else 'serial' if fwd <= RP_SERIAL_FWD else 'table',
                            ends=inext < LO, starts=icur == hi))
            icur = inext
            pos += consumed
            idx += consumed
    if idx > MT_N:
        idx -= MT_N
    return out, idx


def census(nf, shuffles=300, tail=0, all_mixed=False, seed_rank=seed34, seed=1, band_left=0):
    rng = random.Random(seed)
    ref = random.Random(seed)
    perm = list(range(nf))
    chunks, _ = simulate(rng, nf - 1, shuffles, tail=tail, all_mixed=all_mixed, seed_rank=seed_rank, perm=perm,
                         band_left=band_left)
    want = list(range(nf))
    for _ in range(shuffles):
        ref.shuffle(want)
    assert perm == want, 'the chunked draws are random.shuffle'
    n = len(chunks)
    tl = [c for c in chunks if c['mixed']]
    mn = [c for c in chunks if not c['mixed']]

    def mean(xs, key):
        return round(sum(c[key] for c in xs) / len(xs), 3) if xs else None

    return {
        'nf': nf, 'shuffles': shuffles, 'tail': tail, 'all_mixed': all_mixed, 'band_left': band_left,
        'chunks_per_shuffle': round(n / shuffles, 2),
        'tail_chunks_per_shuffle': round(len(tl) / shuffles, 2),
        'chunks_at_icur_le_tail': round(sum(1 for c in chunks if c['icur'] <= tail) / shuffles, 2),
        'jacobi_rounds_per_chunk': mean(chunks, 'rounds'),
        'jacobi_rounds_main': mean(mn, 'rounds'), 'jacobi_rounds_tail': mean(tl, 'rounds'),
        'forwards_per_shuffle': round(sum(c['forwards'] for c in chunks) / shuffles, 2),
        'forwards_per_chunk': mean(chunks, 'forwards'),
        'serial_chunks_per_shuffle': round(sum(c['path'] == 'serial' for c in chunks) / shuffles, 2),
        'table_chunks_per_shuffle': round(sum(c['path'] == 'table' for c in chunks) / shuffles, 2),
        'serial_forwards_per_chunk': mean([c for c in chunks if c['path'] == 'serial'], 'forwards'),
        'table_forwards_per_chunk': mean([c for c in chunks if c['path'] == 'table'], 'forwards'),
        'tail_serial_chunks_per_shuffle': round(sum(c['path'] == 'serial' for c in tl) / shuffles, 2),
        'tail_table_chunks_per_shuffle': round(sum(c['path'] == 'table' for c in tl) / shuffles, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nf', type=int, default=1077, help='floor cells (C3: 1077)')
    ap.add_argument('--tail', type=int, default=0, help='T: chunks at icur <= T take per-lane widths (0: none)')
    ap.add_argument('--all-mixed', action='store_true', help='every chunk takes per-lane widths')
    ap.add_argument('--band-left', type=int, default=0,
                    help='chunks with fewer than this many ranks left in their width band are mixed too (0: none)')
    ap.add_argument('--seed-kind', choices=['34', 'sure'], default='34',
                    help="Jacobi seed: ranks at 3l/4 (the kernel's) or the sure lower bound A_l <= l")
    ap.add_argument('--shuffles', type=int, default=300)
    ap.add_argument('--seed', type=int, default=1)
    a = ap.parse_args()
    print(json.dumps(census(a.nf, a.shuffles, a.tail, a.all_mixed, seed34 if a.seed_kind == '34' else seed_sure,
                            a.seed, a.band_left)))


if __name__ == '__main__':
    main()
