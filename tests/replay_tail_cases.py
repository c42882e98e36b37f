"""The inputs of the replay-tail tests (test_gpu_replay_tail.py on the device, test_replay_tail_cases.py on the
census model): per level and env a seeded MT19937 state, an MT index and a shuffle debt."""
import random
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT / 'tools') not in sys.path:
    sys.path.insert(0, str(ROOT / 'tools'))

TAIL = 95  # MFG_RP_TAIL (csrc/mfg_kernels.h): chunks at icur <= TAIL take per-lane widths
B = 64
MT_IDX = [0, 1, 500, 560, 561, 562, 600, 623, 624]
DEBTS = [1, 2, 3, 5, 8]
BASE_SEED = 20240  # checked on the CPU model: test_replay_tail_cases.py lists what the cases must contain

# (config, variant, floor cells): hi = nf - 1 is the shuffle's first rank
LEVELS = [
    ('tail_hi0.yaml', None, 1),        # the smallest level the spec compiler accepts: a shuffle without a draw
    ('tail_hi1.yaml', None, 2),        # one draw
    ('eight_puzzle.yaml', None, 9),    # hi < TAIL: the whole shuffle in the tail
    ('_obs_test.yaml', None, 80),
    (f'tail_hi{TAIL - 1}.yaml', None, TAIL),
    (f'tail_hi{TAIL}.yaml', None, TAIL + 1),
    (f'tail_hi{TAIL + 1}.yaml', None, TAIL + 2),  # one main-loop draw at least, then the tail
    (f'tail_hi{TAIL + 2}.yaml', None, TAIL + 3),
    ('rooms4.yaml', None, 120),        # the tail after one or two chunks of the main loop
    ('large8.yaml', None, 1077),       # the flagship's floor list
    ('large8.yaml', {'full_temper': 1}, 1077),
]


def env_case(level, env):
    """(624 MT words, mt index, debt) of env `env` of LEVELS[level]; envs 0..44 cover every (index, debt) pair."""
    mt = random.Random(BASE_SEED + 1000 * level + env).getstate()[1][:624]
    return mt, MT_IDX[env % len(MT_IDX)], DEBTS[(env // len(MT_IDX)) % len(DEBTS)]


def cpython(mt, mti):
    r = random.Random()
    r.setstate((3, (*mt, mti), None))
    return r
