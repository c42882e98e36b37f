"""Episode monitoring and state recording over the facade (utils/logging/).

* `EnvMonitor` -- utils/logging/envmonitor.py:14-73: wraps a `Factory`, keeps every step's info dict
  and, at each done, aggregates the episode (columns ending in 'ount' averaged, the others summed,
  IGNORED_DF_COLUMNS dropped, helpers.py:26-28) into one DataFrame row; `save_monitor` pickles the
  DataFrame (our own file, written the way the reference writes it); `auto_plotting_keys` plots the saved
  file with `mfg_amd.plotting.plot_single_run` (utils/plotting/plot_single_runs.py).
* `EnvRecorder` -- utils/logging/recorder.py:10-190: records `summarize_state()` per step for the chosen
  episodes and writes them with the reference's record layout ({'episodes': [{'steps', 'episode_nr'}],
  'n_episodes', 'metadata', 'header'}). The reference serialises that dict through a generated protobuf
  module (utils/proto/fiksProto_pb2), which is not part of this build: records are written as JSON.
  `only_deltas` writes the differences between consecutive episodes (DeepDiff when importable, else a
  built-in structural diff with DeepDiff's report keys); `save_occupation_map` writes the agents' cell-visit
  counts over the level (.npy, plus a .png heatmap when matplotlib is importable; the reference sums into a
  fixed 15x15 array from a key its summary does not have, recorder.py:171-187); `save_trajectory_map` raises
  NotImplementedError like the reference (recorder.py:189-190).
* `BatchedEpisodeLog` -- the batched counterpart: per-episode returns/lengths of a `VectorFactory`,
  collected from its step infos without per-step host copies of the whole batch.
* `BatchedEnvMonitor` -- `EnvMonitor` for a `BatchedFactory` / `VectorFactory`: every env's info dict evaluated
  and folded per episode on the device by one kernel per step (include/mfg_info.h, engine.InfoMonitor);
  `frame()` is the reference's monitor DataFrame with one row per finished episode of any env.
* `BatchedEnvRecorder` -- `EnvRecorder` for a `BatchedFactory`: the chosen envs' per-step states as device rows and
  the whole batch's occupation map, folded by two kernels per step (include/mfg_record.h, engine.StateRecorder);
  `records(env=b)` is the reference's record dict of that env, decoded from the rows (mfg_amd/record_rows.py).
"""
import json
import pickle
from pathlib import Path

IGNORED_DF_COLUMNS = ['Episode', 'Run', 'train_step', 'step', 'index', 'dirt_amount', 'dirty_pos_count',
                      'terminal_observation', 'episode']


class _Wrapper:
    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)


class EnvMonitor(_Wrapper):
    ext = 'png'

    def __init__(self, env, filepath=None):
        super().__init__(env)
        import pandas as pd
        self._pd = pd
        self._filepath = filepath
        self._monitor_df = pd.DataFrame()
        self._monitor_dict = dict()

    def step(self, action):
        obs_type, obs, reward, done, info = self.env.step(action)
        self._read_info(info)
        self._read_done(done)
        return obs_type, obs, reward, done, info

    def reset(self):
        return self.env.reset()

    def _read_info(self, info):
        self._monitor_dict[len(self._monitor_dict)] = {k: v for k, v in info.items()
                                                       if k not in ['terminal_observation', 'episode']}

    def _read_done(self, done):
        if not done:
            return
        pd = self._pd
        df = pd.DataFrame.from_dict(self._monitor_dict, orient='index')
        self._monitor_dict = dict()
        columns = [c for c in df.columns if c not in IGNORED_DF_COLUMNS]
        agg = df.aggregate({c: 'mean' if c.endswith('ount') else 'sum' for c in columns})
        agg['episode'] = len(self._monitor_df)
        self._monitor_df = pd.concat([self._monitor_df, pd.DataFrame([agg])], ignore_index=True)

    @property
    def monitor_df(self):
        return self._monitor_df

    def save_monitor(self, filepath=None, auto_plotting_keys=None):
        filepath = Path(filepath or self._filepath)
        filepath.parent.mkdir(exist_ok=True, parents=True)
        with filepath.open('wb') as f:
            pickle.dump(self._monitor_df.reset_index(), f, protocol=pickle.HIGHEST_PROTOCOL)
        if auto_plotting_keys:
            from .plotting import plot_single_run
            plot_single_run(filepath, column_keys=auto_plotting_keys)

    def report_possible_colum_keys(self):
        print(self._monitor_df.columns)


class EnvRecorder(_Wrapper):
    def __init__(self, env, filepath=None, episodes=None):
        super().__init__(env)
        self.filepath = filepath
        self.episodes = episodes
        self._curr_episode = 0
        self._curr_ep_recorder = list()
        self._recorder_out_list = list()

    def reset(self):
        self._curr_ep_recorder = list()
        self._recorder_out_list = list()
        self._curr_episode += 1
        return self.env.reset()

    def step(self, actions):
        obs_type, obs, reward, done, info = self.env.step(actions)
        if not self.episodes or self._curr_episode in self.episodes:
            self._curr_ep_recorder.append(self.env.summarize_state())
            if done:
                self._recorder_out_list.append({'steps': self._curr_ep_recorder, 'episode_nr': self._curr_episode})
                self._curr_ep_recorder = list()
        return obs_type, obs, reward, done, info

    def _finalize(self):
        if self._curr_ep_recorder:
            self._recorder_out_list.append({'steps': self._curr_ep_recorder.copy(),
                                            'episode_nr': len(self._recorder_out_list)})

    def records(self):
        """The record dict save_records writes (recorder.py:96-158 layout)."""
        params = self.env.params
        return {'episodes': self._recorder_out_list, 'n_episodes': self._curr_episode,
                'metadata': dict(level_name=params['General']['level_name'], n_agents=len(params['Agents']),
                                 env_seed=params['General'].get('env_seed', 69),
                                 pomdp_r=params['General']['pomdp_r'], individual_rewards=True),
                'header': self.env.summarize_header()}

    def save_records(self, filepath=None, only_deltas=False, save_occupation_map=False, save_trajectory_map=False):
        self._finalize()
        filepath = Path(filepath or self.filepath)
        filepath.parent.mkdir(exist_ok=True, parents=True)
        rec = self.records()
        if only_deltas:
            eps = rec['episodes']
            rec['episodes'] = [_deltas(a, b) for a, b in zip(eps, eps[1:])]
        with filepath.open('w') as f:
            json.dump(rec, f, default=str)
        if save_occupation_map:
            self.occupation_map(filepath.with_name(filepath.stem + '_occupation'))
        if save_trajectory_map:
            raise NotImplementedError('This has not yet been implemented.')  # as the reference (recorder.py:189-190)
        return filepath

    def occupation_map(self, out_stem=None):
        """[H, W] counts of agent positions over every recorded step (recorder.py:171-180, over the level's
        shape); with out_stem, written to <out_stem>.npy and, if matplotlib is importable, <out_stem>.png."""
        import numpy as np
        H, W = self.env.spec.H, self.env.spec.W
        occ = np.zeros((H, W), np.int64)
        for ep in self._recorder_out_list:
            for st in ep['steps']:
                for a in st.get('agents', []):
                    if 0 <= a['x'] < H and 0 <= a['y'] < W:
                        occ[a['x'], a['y']] += 1
        return _write_occupation(occ, out_stem)


def _write_occupation(occ, out_stem=None):
    """With out_stem: the [H, W] map to <out_stem>.npy and, if matplotlib is importable, a heatmap to
    <out_stem>.png. Returns the map."""
    import numpy as np
    H, W = occ.shape
    if out_stem is not None:
        out_stem = Path(out_stem)
        np.save(out_stem.with_suffix('.npy'), occ)
        try:
            import matplotlib
            matplotlib.use('Agg')
            import matplotlib.pyplot as plt
        except Exception:
            return occ
        fig, ax = plt.subplots(figsize=(6, 6 * H / max(W, 1) + 0.5))
        im = ax.imshow(occ, cmap='viridis')
        fig.colorbar(im, ax=ax)
        ax.set_title('agent occupation')
        fig.savefig(out_stem.with_suffix('.png'))
        plt.close(fig)
    return occ


def _deltas(t1, t2):
    """Differences between two episode records: DeepDiff(t1, t2, ignore_order=True) (recorder.py:91-95) when
    deepdiff is importable, else a structural diff reporting DeepDiff's keys for ordered data
    (values_changed, type_changes, dictionary_item_added/removed, iterable_item_added/removed)."""
    try:
        from deepdiff import DeepDiff
        return json.loads(DeepDiff(t1, t2, ignore_order=True).to_json())
    except ImportError:
        pass
    out = {}

    def put(kind, path, val):
        out.setdefault(kind, {})[path] = val

    def walk(a, b, path):
        if isinstance(a, dict) and isinstance(b, dict):
            for k in a:
                if k not in b:
                    put('dictionary_item_removed', f"{path}['{k}']", a[k])
                else:
                    walk(a[k], b[k], f"{path}['{k}']")
            for k in b:
                if k not in a:
                    put('dictionary_item_added', f"{path}['{k}']", b[k])
        elif isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
            for i in range(min(len(a), len(b))):
                walk(a[i], b[i], f'{path}[{i}]')
            for i in range(len(b), len(a)):
                put('iterable_item_removed', f'{path}[{i}]', a[i])
            for i in range(len(a), len(b)):
                put('iterable_item_added', f'{path}[{i}]', b[i])
        elif type(a) is not type(b):
            put('type_changes', path, {'old_type': type(a).__name__, 'new_type': type(b).__name__,
                                       'old_value': a, 'new_value': b})
        elif a != b:
            put('values_changed', path, {'old_value': a, 'new_value': b})

    walk(t1, t2, 'root')
    return out


def episode_frame(program, hdr, sums, counts):
    """Finished-episode rows of the info monitor (include/mfg_info.h: header i32 [n, 8], sum f64 [n, Kc], count
    u32 [n, Kc]) as the reference's monitor DataFrame (EnvMonitor._read_done): per episode, every info key present at
    least once is summed, or averaged over the steps where it was present if it ends in 'ount'; IGNORED_DF_COLUMNS
    are dropped; a key absent in an episode is NaN. Adds 'env', 'episode' (that env's episode index) and 'length'."""
    import pandas as pd
    from .info_program import HDR_ENV, HDR_EP_INDEX, HDR_LENGTH, HDR_MAINT_BASE
    rows = []
    for i in range(len(hdr)):
        row = {'env': int(hdr[i][HDR_ENV]), 'episode': int(hdr[i][HDR_EP_INDEX]), 'length': int(hdr[i][HDR_LENGTH])}
        for k in counts[i].nonzero()[0]:
            name = program.column_name(int(k), hdr[i][HDR_MAINT_BASE])
            if name in IGNORED_DF_COLUMNS:
                continue
            v = float(sums[i][k])
            row[name] = v / int(counts[i][k]) if name.endswith('ount') else v
        rows.append(row)
    if not rows:
        return pd.DataFrame(columns=['env', 'episode', 'length'])
    return pd.DataFrame(rows)


class BatchedEnvMonitor(_Wrapper):
    """`EnvMonitor` for the batched engine: wraps a `BatchedFactory` or a `VectorFactory`; every step's info columns
    are evaluated and folded per episode on the device (engine.InfoMonitor, one kernel on the env's stream, no host
    sync and no per-step device->host copy). Finished episodes wait in a device buffer of `ep_capacity` rows until
    `drain()` / `frame()` fetch them; episodes finishing while it is full are counted in `dropped`."""

    def __init__(self, env, filepath=None, ep_capacity=None):
        super().__init__(env)
        from .engine import InfoMonitor
        from .info_program import compile_info_program
        self._vector = hasattr(env, 'num_envs')  # a VectorFactory keeps its BatchedFactory in .env
        self._bf = env.env if self._vector else env
        bf = self._bf
        torch = bf.torch
        self._filepath = filepath
        self.program = compile_info_program(bf.spec)
        self.monitor = InfoMonitor(self.program, bf.B, device=bf.device, ep_capacity=ep_capacity)
        Kc = self.monitor.Kc
        self._vals = torch.zeros((1, bf.B, Kc), dtype=torch.float64, device=bf.device)
        self._pres = torch.zeros((1, bf.B, Kc), dtype=torch.uint8, device=bf.device)
        self._hdr, self._sum, self._cnt = [], [], []
        self.dropped = 0

    def step(self, actions):
        bf = self._bf
        out = self.env.step(actions)
        a = actions.to(device=bf.device, dtype=bf.torch.int32).contiguous()
        self.monitor.step(1, bf.ev_act, bf.ev_watch, bf.ev_misc, bf.reward, bf.done, actions=a, vals=self._vals,
                          pres=self._pres)
        return out

    def reset(self, mask=None, **kw):
        """Forwarded to the env (a VectorFactory takes the mask as options={'mask': ...}); the masked envs' episode
        accumulators restart (all envs without a mask)."""
        bf = self._bf
        m = None if mask is None else mask.to(device=bf.device, dtype=bf.torch.uint8).contiguous()
        if self._vector:
            out = self.env.reset(options=None if m is None else {'mask': m}, **kw)
        else:
            out = self.env.reset(mask=m, **kw)
        self.monitor.reset(m)
        return out

    def step_columns(self):
        """The last step's (names, values f64 [B, Kc], present bool [B, Kc]) on the device, as
        `BatchedFactory.info_columns` returns them (a crashed env's row is 0 / absent)."""
        return self.program.columns, self._vals[0], self._pres[0].bool()

    def drain(self):
        """Fetch the finished episodes from the device (one sync): host tensors env / episode / length / crashed /
        maint_base [n], sum f64 [n, Kc], count i64 [n, Kc], sorted by (env, episode), and `dropped`, the number of
        episodes that found the device buffer full since the last drain. The rows also feed `frame()`."""
        import numpy as np
        from .info_program import HDR_ENV, HDR_EP_INDEX, HDR_LENGTH, HDR_CRASHED, HDR_MAINT_BASE
        torch = self._bf.torch
        hdr, s, c, dropped = self.monitor.drain()
        self._hdr.append(hdr)
        self._sum.append(s)
        self._cnt.append(c)
        self.dropped += dropped
        col = lambda j: torch.from_numpy(np.ascontiguousarray(hdr[:, j]))
        return {'env': col(HDR_ENV), 'episode': col(HDR_EP_INDEX), 'length': col(HDR_LENGTH),
                'crashed': col(HDR_CRASHED), 'maint_base': col(HDR_MAINT_BASE), 'sum': torch.from_numpy(s),
                'count': torch.from_numpy(c.astype(np.int64)), 'dropped': dropped}

    def frame(self):
        """One row per finished episode so far (drains first), in drain order: see `episode_frame`."""
        import numpy as np
        self.drain()
        return episode_frame(self.program, np.concatenate(self._hdr), np.concatenate(self._sum),
                             np.concatenate(self._cnt))

    @property
    def monitor_df(self):
        return self.frame()

    def save_monitor(self, filepath=None):
        filepath = Path(filepath or self._filepath)
        filepath.parent.mkdir(exist_ok=True, parents=True)
        with filepath.open('wb') as f:
            pickle.dump(self.frame().reset_index(), f, protocol=pickle.HIGHEST_PROTOCOL)

    def close(self):
        self.monitor.close()
        self.env.close()


class BatchedEnvRecorder(_Wrapper):
    """`EnvRecorder` for a `BatchedFactory` (any obs_dtype): the state of the selected `envs` after every step, kept
    on the device as fixed-width rows (engine.StateRecorder, include/mfg_record.h), and with `occupancy` the cell-visit
    counts of the agents of ALL envs; no per-step host copy and no host sync.

    `step` splits the factory's step so that a done step's state can still be read: the engine steps without
    auto-reset, the recorder kernel reads the records, then the done envs are reset and the observations rendered,
    all on the factory's stream. What it returns equals `BatchedFactory.step`, value for value.

    Rows wait in a device ring of `capacity` rows per selected env. With `auto_drain` the wrapper fetches them before
    the ring could fill (one drain, and one sync, per `capacity` steps); with `auto_drain=False` draining is the
    caller's (`drain()`), and rows that found the ring full are counted in `dropped` (`dropped_by_env` per env).
    `episodes`: record only these 1-based episode numbers of each env (the reference's `episodes` list).

    Departure from the reference: `EnvRecorder` forgets its episode list at every `reset()` (recorder.py:35-36) and
    numbers an unfinished tail `len(list)` (:63-66). Here every recorded episode is kept and `episode_nr` is always
    the env's own 1-based episode number, for an unfinished tail too. A crashed step (a reference crash path) has no
    state in the reference: it closes the episode without a step dict and counts in `crashed_steps`."""

    def __init__(self, env, envs, filepath=None, episodes=None, capacity=256, occupancy=True, auto_drain=True,
                 occ_lds_cells=0):
        from .engine import check_record_args
        ids, capacity, _ = check_record_args(env.B, envs, capacity, episodes)  # before any device work
        super().__init__(env)
        from .engine import StateRecorder
        self.filepath = filepath
        self.envs = [int(b) for b in ids]
        self.episodes = list(episodes) if episodes else None
        self.capacity = capacity
        self.auto_drain = bool(auto_drain)
        self.recorder = StateRecorder(env.engine, ids, capacity=capacity, episodes=episodes, occupancy=occupancy,
                                      occ_lds_cells=occ_lds_cells)
        self._rows = {b: [] for b in self.envs}  # per env: drained row blocks, in step order
        self._since_drain = 0
        self.dropped = 0
        self.dropped_by_env = {b: 0 for b in self.envs}

    def reset(self, mask=None):
        return self.env.reset(mask=mask)

    def step(self, actions):
        bf = self.env
        if not bf._created:
            raise RuntimeError('call reset() first')
        a = actions.to(device=bf.device, dtype=bf.torch.int32).contiguous()
        if a.shape != (bf.B, bf.spec.n_agents):
            raise ValueError(f'actions must be [{bf.B}, {bf.spec.n_agents}]')
        if self.auto_drain and self._since_drain >= self.capacity:
            self.drain()
        bf.engine.step(1, actions=a, reward=bf.reward, done=bf.done, obs=None, ev_act=bf.ev_act, ev_watch=bf.ev_watch,
                       ev_misc=bf.ev_misc, auto_reset=False, step_base=bf.t)
        self.recorder.step(a, bf.ev_act, bf.ev_watch, bf.ev_misc, bf.done)
        # a masked reset renders the observations of every env (include/mfg.h, mfg_reset)
        bf.engine.reset(obs=bf.obs, mask=bf.done, init=0)
        bf.t += 1
        self._since_drain += 1
        return bf.obs, bf.reward, bf.done, (bf.ev_act, bf.ev_watch, bf.ev_misc)

    def drain(self):
        """Fetch the rows recorded since the last drain (one sync); returns the number of rows dropped since then."""
        rows, counts = self.recorder.drain()
        lost = 0
        for s, b in enumerate(self.envs):
            n = min(int(counts[s]), self.capacity)
            if n:
                self._rows[b].append(rows[s, :n].copy())
            self.dropped_by_env[b] += int(counts[s]) - n
            lost += int(counts[s]) - n
        self.dropped += lost
        self._since_drain = 0
        return lost

    def rows(self, env):
        """uint32 [n, row_words]: every row of env `env` recorded so far, in step order (drains first)."""
        import numpy as np
        if env not in self._rows:
            raise KeyError(f'env {env} is not recorded (recorded: {self.envs})')
        self.drain()
        blocks = self._rows[env]
        if len(blocks) > 1:
            self._rows[env] = blocks = [np.concatenate(blocks)]
        return blocks[0] if blocks else np.zeros((0, self.recorder.row_words), np.uint32)

    def _episodes(self, env):
        """([{'steps': [...], 'episode_nr': n}], crashed steps) of env's rows: every step dict is
        `views.summarize_state` of the row's `Snapshot`."""
        from . import views
        from .record_rows import row_fields, row_snapshot
        spec, layout = self.env.spec, self.env.engine.layout
        out, cur, cur_nr, crashed_steps = [], [], None, 0

        def close():
            nonlocal cur
            if cur:
                out.append({'steps': cur, 'episode_nr': cur_nr})
            cur = []

        for row in self.rows(env):
            _, ep, _, done, crashed = row_fields(row)
            if cur_nr is not None and ep != cur_nr:  # (an episode the filter cut short, or a caller's reset)
                close()
            cur_nr = ep
            if crashed:
                crashed_steps += 1
                close()
                continue
            cur.append(views.summarize_state(spec, row_snapshot(spec, layout, row)))
            if done:
                close()
        close()
        return out, crashed_steps

    def _record_view(self, env):
        from .engine import RecordView
        return RecordView(self.recorder.env_state(env), self.env.engine.layout, self.env.spec)

    def records(self, env):
        """`EnvRecorder.records()`'s dict for one recorded env: {'episodes', 'n_episodes', 'metadata', 'header'}, plus
        'crashed_steps'. The header is `views.summarize_header` of the env's current record (one host copy)."""
        from . import views
        import yaml
        episodes, crashed_steps = self._episodes(env)
        view = self._record_view(env)
        with open(self.env.spec.config_path) as f:
            params = yaml.safe_load(f)
        return {'episodes': episodes, 'n_episodes': view.hdr('episode') + 1,
                'metadata': dict(level_name=params['General']['level_name'], n_agents=len(params['Agents']),
                                 env_seed=params['General'].get('env_seed', 69),
                                 pomdp_r=params['General']['pomdp_r'], individual_rewards=True),
                'header': views.summarize_header(self.env.spec, views.snapshot_from_record(view, None)),
                'crashed_steps': crashed_steps}

    @property
    def crashed_steps(self):
        return sum(self._episodes(b)[1] for b in self.envs)

    def save_records(self, filepath=None, env=None, only_deltas=False, save_occupation_map=False,
                     save_trajectory_map=False):
        """JSON like `EnvRecorder.save_records`; env=None writes one file per recorded env, '_env{b}' in the stem.
        Returns the path (or the list of paths)."""
        filepath = Path(filepath or self.filepath)
        filepath.parent.mkdir(exist_ok=True, parents=True)
        paths = []
        for b in (self.envs if env is None else [env]):
            rec = self.records(b)
            if only_deltas:
                eps = rec['episodes']
                rec['episodes'] = [_deltas(x, y) for x, y in zip(eps, eps[1:])]
            path = filepath if env is not None else filepath.with_name(f'{filepath.stem}_env{b}{filepath.suffix}')
            with path.open('w') as f:
                json.dump(rec, f, default=str)
            paths.append(path)
        if save_occupation_map:
            self.occupation_map(filepath.with_name(filepath.stem + '_occupation'))
        if save_trajectory_map:
            raise NotImplementedError('This has not yet been implemented.')  # as the reference (recorder.py:189-190)
        return paths[0] if env is not None else paths

    def occupation_map(self, out_stem=None):
        """[H, W] int64 counts of the agents' positions over every env of the batch and every step since the last
        `clear_occupation()`; written like `EnvRecorder.occupation_map` with out_stem."""
        import numpy as np
        spec = self.env.spec
        occ = self.recorder.occupancy_map().astype(np.int64).reshape(spec.H, spec.W)
        return _write_occupation(occ, out_stem)

    def clear_occupation(self):
        self.recorder.clear_occupancy()

    def trajectory(self, env, episode):
        """int array [T, A, 2]: the agents' (x, y) over the recorded steps of env's episode `episode` (1-based)."""
        import numpy as np
        from .record_rows import row_cells, row_fields
        spec, layout = self.env.spec, self.env.engine.layout
        cells = [row_cells(spec, layout, r) for r in self.rows(env) if row_fields(r)[1] == episode]
        if not cells:
            return np.zeros((0, spec.n_agents, 2), np.int64)
        c = np.stack(cells).astype(np.int64)
        return np.stack([c // spec.W, c % spec.W], axis=-1)

    def close(self):
        self.recorder.close()
        self.env.close()


class BatchedEpisodeLog:
    """Finished-episode statistics of a `VectorFactory`: call `update(infos)` after each step."""

    def __init__(self):
        self.returns, self.lengths, self.env_ids = [], [], []

    def update(self, infos):
        if '_final' not in infos:
            return 0
        idx = infos['_final'].nonzero().flatten()
        if idx.numel() == 0:
            return 0
        self.returns.append(infos['final_return'][idx].cpu())
        self.lengths.append(infos['final_length'][idx].cpu())
        self.env_ids.append(idx.cpu())
        return int(idx.numel())

    def frame(self):
        import pandas as pd
        import torch
        if not self.returns:
            return pd.DataFrame(columns=['env', 'length', 'return_sum'])
        r = torch.cat(self.returns)
        df = pd.DataFrame({'env': torch.cat(self.env_ids).numpy(), 'length': torch.cat(self.lengths).numpy(),
                           'return_sum': r.sum(dim=1).numpy()})
        for a in range(r.shape[1]):
            df[f'return_{a}'] = r[:, a].numpy()
        return df
