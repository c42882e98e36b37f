"""The ctypes binding of include/mfg_learn.h: the learner-side and evaluation kernels of libmfg_hip.so (csrc/mfg_learn.hip,
mfg_ppo.hip, mfg_seac.hip, mfg_act.hip). One table for all of the header's functions, bound once on the engine's
library handle; tests/test_spec_abi.py checks the table against the header's prototypes."""
import ctypes as C

import torch

_p, _i64, _i32, _f32 = C.c_void_p, C.c_int64, C.c_int, C.c_float

# function -> argtypes, in the header's order; every function returns int (0, or -1 on a bad size or launch error)
ARGTYPES = {
    'mfg_gru_fwd_step': [_p, _i64, _p, _p, _p, _i64, _p, _i64, _p, _i64, _p, _p, _p, _p, _p, _i64, _i64, _i32, _p],
    'mfg_gru_bwd_step': [_p, _i64, _p, _p, _i64, _p, _p, _p, _p, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _i32, _p],
    'mfg_packed_densify': [_p, _p, _i64, _i32, _i32, _p, _i64, _p],
    'mfg_packed_project': [_p, _p, _i64, _i32, _p, _p, _i32, _i32, _p, _i64, _p],
    'mfg_sample_categorical': [_p, _i64, _i32, _p, _i64, _p, _p],
    'mfg_mc_returns': [_p, _i64, _p, _i64, _i64, _i32, _f32, _p, _i64, _p, _p, _p],
    'mfg_ppo_head': [_p, _i64, _p, _i64, _p, _p, _p, _p, _i64, _i32, _f32, _f32, _f32, _p, _p, _i64, _p, _p, _p],
    'mfg_packed_project_grouped': [_p, _p, _i64, _i32, _i32, _p, _p, _i32, _i32, _i32, _p, _i64, _p],
    'mfg_gru_fwd_step_grouped': [_p, _i64, _p, _p, _i64, _p, _i64, _p, _i64, _p, _i64, _p, _p, _p, _p, _p, _i64, _i64,
                                 _i32, _p],
    'mfg_seac_head': [_p, _p, _i32, _i64, _i32, _i32, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64,
                      _p, _f32, _f32, _f32, _f32, _i32, _p, _p, _p, _p, _p],
    'mfg_policy_act': [_p, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _i64, _i64, _p,
                       _i32, _p, _p, _p],
    'mfg_eval_fold': [_p, _p, _i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _p],
}

# include/mfg_act.h, bound the same way
ACT_ARGTYPES = {
    'mfg_policy_act_masked': [_p, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _i64, _i64,
                              _p, _i32, _p, _p, _p, _p],
}

ACTOR_FIELDS = ('action_emb', 'w1t', 'b1', 'w3t', 'b3', 'wiht', 'bih', 'whht', 'bhh', 'wat', 'ba', 'wbt', 'bb')


class ActorWeights(C.Structure):
    """mfg_actor_weights: device pointers of the stacked actor parameters (mfg_policy_act)."""
    _fields_ = [(k, C.c_void_p) for k in ACTOR_FIELDS]


_LIB = None


def lib():
    """libmfg_hip.so with every function of include/mfg_learn.h and include/mfg_act.h bound (once)."""
    global _LIB
    if _LIB is None:
        from .engine import load_lib
        L = load_lib()
        for name, argtypes in {**ARGTYPES, **ACT_ARGTYPES}.items():
            fn = getattr(L, name)  # a library without the function is an error here, not at its first use
            fn.argtypes, fn.restype = argtypes, C.c_int
        _LIB = L
    return _LIB


def call(name, *args):
    """Call a function of the table; a non-zero return (bad size, launch error) raises."""
    if getattr(lib(), name)(*args):
        raise RuntimeError(f'{name} failed')


def stream(dev):
    """The current HIP stream of ``dev`` as the integer the kernels' ``void* stream`` takes."""
    return torch.cuda.current_stream(dev).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()
