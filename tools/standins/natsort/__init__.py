"""Stand-in: `natsorted` orders strings (or paths) so that runs of digits compare as numbers ('agent_2' before
'agent_10'), which is all the reference's iac.py asks of it."""
import re


def _key(x):
    return [int(p) if p.isdigit() else p.lower() for p in re.split(r'(\d+)', str(x))]


def natsorted(seq, key=None, reverse=False):
    return sorted(seq, key=(lambda x: _key(key(x))) if key else _key, reverse=reverse)
