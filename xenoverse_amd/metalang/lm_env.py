"""MetaLMV3 on the device (csrc/metalm.hip, C-ABI xv_metalm_*): MetaLMV3VecEnv steps many query/answer/reward envs in one
launch; MetaLMV3Env puts the reference's scalar surface (xenoverse/metalang/metalangv3.py:4-42) on a batch of one."""
import ctypes as C

import numpy as np

from .. import _lib
from .lm_host import RandomLMHost, check_lm_limit

XV_DEVERR_LENGTH = 16      # include/xeno.h: a pass reached max_len tokens without the stop token


def _lm_of(task, what):
    if not isinstance(task, dict) or "lm" not in task:
        raise ValueError("%s: a task is the dict TaskSamplerV3 returns (key 'lm')" % what)
    lm = task["lm"]
    return lm if isinstance(lm, RandomLMHost) else RandomLMHost.from_reference(lm)


def env_task_of(n_task, num_envs, env_task_index=None):
    """the task of every env as int32 [num_envs]: the given indices, checked, or the default (the only task; task i for
    env i when there are num_envs tasks)"""
    if env_task_index is None:
        if n_task == 1:
            env_task_index = np.zeros(num_envs, np.int32)
        elif n_task == num_envs:
            env_task_index = np.arange(num_envs, dtype=np.int32)
        else:
            raise ValueError("%d tasks for %d envs: give env_task_index" % (n_task, num_envs))
    if hasattr(env_task_index, "detach"):
        env_task_index = env_task_index.detach().cpu().numpy()
    eti = np.ascontiguousarray(env_task_index, dtype=np.int32)
    if eti.shape != (num_envs,) or eti.min() < 0 or eti.max() >= n_task:
        raise ValueError("env_task_index must be int[num_envs] with values in [0, %d)" % n_task)
    return eti


def tables_for_set_task(tables, device):
    """the tables dict of metalang.sample_tasks_device -> ([emb, w_h_t, b_h, w_d_t, b_d] as the handle borrows them, n_task,
    (V, E, H, stop, function tokens)).  A float64, contiguous tensor already on `device` is taken as it is."""
    import torch
    from .device_sampler import TABLE_KEYS, function_tokens
    emb = tables["emb"]
    if not torch.is_tensor(emb) or emb.dim() != 3 or emb.shape[0] < 1:
        raise ValueError("tables['emb'] must be a tensor [n_task, V, E]")
    n, V, E = (int(v) for v in emb.shape)
    H = int(tables["b_h"].shape[-1])
    shapes = dict(emb=(n, V, E), w_h_t=(n, H + E, H), b_h=(n, H), w_d_t=(n, H, V), b_d=(n, V))
    dev = []
    for k in TABLE_KEYS:
        t = tables[k]
        if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != shapes[k]:
            raise ValueError("tables[%r] must be a float64 tensor of shape %s" % (k, shapes[k]))
        dev.append(t.to(device).contiguous())
    for k, v in (("vocabulary", V), ("embedding", E), ("hidden", H)):
        if k in tables and int(tables[k]) != v:
            raise ValueError("tables[%r] = %d, the tensors say %d" % (k, int(tables[k]), v))
        check_lm_limit({"vocabulary": "n_vocab", "embedding": "n_emb", "hidden": "n_hidden"}[k], v)
    stop, fun = function_tokens(tables.get("function_vocabulary"))
    return dev, n, (V, E, H, stop, tuple(fun))


class MetaLMV3VecEnv(object):
    """num_envs envs, each one RandomLM task with its current query and the hidden state that query left.  Every task of a
    handle has the same (vocabulary, embedding, hidden), stop token and function tokens.

    Token rows are int32 [num_envs, max_len] on the device, padded with 0 behind their length (the label row has
    max_len + 1 entries: one per answer position and one for the stop position).  A pass that emits max_len tokens and
    then does not draw the stop token is cut there and sets XV_DEVERR_LENGTH in check_errors().

    Free-running draws are Philox, keyed by (seed, env_id_base + env, the engine's tick at the call, pass, position): a
    handle over envs [e0, e1) made with env_id_base + e0 draws what the whole batch draws there.  reset(), policy() and
    step() each advance the tick by one.  draws=: a dict of injected uniforms float64 [num_envs, max_len + 1] per pass
    (u_query, u_policy, u_greedy, u_low), one per token in the order numpy.random.choice would consume them (the parity
    path); a pass without an entry draws from Philox.

    truncated = steps >= max_steps (the reference's scalar env returns steps < max_steps in that place: MetaLMV3Env)."""

    def __init__(self, num_envs, max_len=1024, max_steps=10000, device="cuda:0", seed=0, env_id_base=0):
        from ..engine import Engine
        if int(num_envs) < 1:
            raise ValueError("num_envs must be at least 1")
        check_lm_limit("max_len", max_len)
        self.num_envs, self.max_len, self.max_steps = int(num_envs), int(max_len), int(max_steps)
        self._h = None
        self.engine = Engine(device, seed=seed, env_id_base=env_id_base)
        self.lib, self.device = self.engine.lib, self.engine.device
        self._tables = None
        self._sizes = None

    # ---- tasks ----------------------------------------------------------------------------------------------------
    def set_task(self, tasks, env_task_index=None):
        """tasks: one task dict (TaskSamplerV3), a list of them, or the tables dict of metalang.sample_tasks_device, whose
        device tensors the handle borrows as they are (no host copy, no RandomLMHost objects); env_task_index
        int[num_envs]: the task of every env (default: the only task; task i for env i when there are num_envs tasks)"""
        import torch
        from .device_sampler import is_tables
        if is_tables(tasks):
            dev, n_task, sizes = tables_for_set_task(tasks, self.device)
        else:
            if isinstance(tasks, dict):
                tasks = [tasks]
            if not len(tasks):
                raise ValueError("set_task needs at least one task")
            lms = [_lm_of(t, "task %d" % k) for k, t in enumerate(tasks)]
            V, E, H = lms[0].n_vocab, lms[0].n_emb, lms[0].n_hidden
            stop, fun = lms[0].stop_token, sorted(lms[0].function_token_list)
            for k, lm in enumerate(lms):
                if (lm.n_vocab, lm.n_emb, lm.n_hidden) != (V, E, H):
                    raise ValueError("task %d has (vocabulary, embedding, hidden) = %s, task 0 has %s: one handle holds one "
                                     "size" % (k, (lm.n_vocab, lm.n_emb, lm.n_hidden), (V, E, H)))
                if lm.stop_token != stop or sorted(lm.function_token_list) != fun:
                    raise ValueError("task %d has other stop / function tokens than task 0" % k)
            n_task = len(lms)
            host = [np.stack([lm.emb for lm in lms]),
                    np.stack([lm.rnn_w.T for lm in lms]),      # [H + E][H]: the lanes of a wave own rows of W_h
                    np.stack([lm.rnn_b for lm in lms]),
                    np.stack([lm.dec_w.T for lm in lms]),      # [H][V]: and columns of the logits
                    np.stack([lm.dec_b for lm in lms])]
            dev = [torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in host]
            sizes = (V, E, H, stop, tuple(fun))
        dev.append(torch.from_numpy(env_task_of(n_task, self.num_envs, env_task_index)).to(self.device))
        V, E, H, stop, fun = sizes
        if self._h is not None and sizes != self._sizes:
            self._destroy()
        if self._h is None:
            h = C.c_void_p()
            ft = (C.c_int32 * max(len(fun), 1))(*fun)
            _lib.check(self.lib.xv_metalm_create(self.engine.handle, self.num_envs, V, E, H, self.max_len, stop, ft, len(fun),
                                                 C.byref(h)))
            self._h = h
        self.engine.sync()      # the tables a running call reads are let go below
        _lib.check(self.lib.xv_metalm_set_task(self._h, n_task, *(_lib.ptr(t) for t in dev)))
        self._tables = dev      # borrowed by the handle
        self._sizes = sizes
        self.n_vocab, self.n_emb, self.n_hidden, self.n_task = V, E, H, n_task

    def _live(self):
        if self._h is None:
            raise Exception("Task not set")      # the reference's text (metalangv3.py:23)

    def _draw(self, draws, key):
        import torch
        if draws is None or draws.get(key) is None:
            return None
        u = torch.as_tensor(draws[key], dtype=torch.float64).to(self.device).contiguous()
        if tuple(u.shape) != (self.num_envs, self.max_len + 1):
            raise ValueError("draws[%r] must have shape %s, got %s" % (key, (self.num_envs, self.max_len + 1), tuple(u.shape)))
        return u

    def _tokens(self, extra=0):
        import torch
        return (torch.empty((self.num_envs, self.max_len + extra), dtype=torch.int32, device=self.device),
                torch.empty(self.num_envs, dtype=torch.int32, device=self.device))

    # ---- the env ----------------------------------------------------------------------------------------------------
    def reset(self, draws=None):
        """-> (query int32 [num_envs, max_len], query_len int32 [num_envs])"""
        self._live()
        u = self._draw(draws, "u_query")
        query, query_len = self._tokens()
        _lib.check(self.lib.xv_metalm_reset(self._h, _lib.ptr(u), _lib.ptr(query), _lib.ptr(query_len)))
        return query, query_len

    def policy(self, T=1.0, draws=None):
        """a softmax answer at temperature T (a scalar or [num_envs]) -> (answer, answer_len)"""
        import torch
        self._live()
        if np.ndim(T) == 0 and not torch.is_tensor(T):
            temp = torch.full((self.num_envs,), float(T), dtype=torch.float64, device=self.device)
        else:
            temp = torch.as_tensor(T, dtype=torch.float64).to(self.device).contiguous()
            if tuple(temp.shape) != (self.num_envs,):
                raise ValueError("T must be a scalar or have shape (%d,)" % self.num_envs)
        u = self._draw(draws, "u_policy")
        answer, answer_len = self._tokens()
        _lib.check(self.lib.xv_metalm_policy(self._h, _lib.ptr(temp), _lib.ptr(u), _lib.ptr(answer), _lib.ptr(answer_len)))
        return answer, answer_len

    def step(self, answer, answer_len, cached=False, draws=None):
        """-> obs = (query, query_len), reward float64 [num_envs], terminated, truncated, info.  cached: False, True or
        bool[num_envs]: an env with cached set keeps its query and its cached state.  info: label [num_envs, max_len + 1]
        (answer_len + 1 entries), ppl, ppl_min, ppl_max, greedy / low answers with greedy_len / low_len, steps."""
        import torch
        self._live()
        ans = torch.as_tensor(answer).to(self.device, torch.int32).contiguous()
        alen = torch.as_tensor(answer_len).to(self.device, torch.int32).contiguous()
        if tuple(ans.shape) != (self.num_envs, self.max_len) or tuple(alen.shape) != (self.num_envs,):
            raise ValueError("answer must have shape (%d, %d) and answer_len (%d,)" % (self.num_envs, self.max_len,
                                                                                        self.num_envs))
        mask = None
        if not (np.ndim(cached) == 0 and not torch.is_tensor(cached) and not cached):
            if np.ndim(cached) == 0 and not torch.is_tensor(cached):
                mask = torch.ones(self.num_envs, dtype=torch.uint8, device=self.device)
            else:
                mask = torch.as_tensor(cached).to(self.device).to(torch.uint8).contiguous()
                if tuple(mask.shape) != (self.num_envs,):
                    raise ValueError("cached must be a bool or have shape (%d,)" % self.num_envs)
        us = [self._draw(draws, k) for k in ("u_greedy", "u_low", "u_query")]
        query, query_len = self._tokens()
        label, _ = self._tokens(1)
        greedy, greedy_len = self._tokens()
        low, low_len = self._tokens()
        reward = torch.empty(self.num_envs, dtype=torch.float64, device=self.device)
        ppl = torch.empty((3, self.num_envs), dtype=torch.float64, device=self.device)
        steps = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.xv_metalm_step(self._h, _lib.ptr(ans), _lib.ptr(alen), _lib.ptr(mask), *(_lib.ptr(u) for u in us),
                                           _lib.ptr(query), _lib.ptr(query_len), _lib.ptr(reward), _lib.ptr(steps),
                                           _lib.ptr(label), _lib.ptr(ppl), _lib.ptr(greedy), _lib.ptr(greedy_len),
                                           _lib.ptr(low), _lib.ptr(low_len)))
        terminated = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        info = dict(label=label, ppl=ppl[0], ppl_min=ppl[1], ppl_max=ppl[2], greedy=greedy, greedy_len=greedy_len, low=low,
                    low_len=low_len, steps=steps)
        return (query, query_len), reward, terminated, steps >= self.max_steps, info

    # ---- the training streams ---------------------------------------------------------------------------------------
    def stream(self, datatype, L, T_choices=None, t_index=None, max_rounds=None, draws=None):
        """The reference's generate_data_v3_single_task_qa / _qar / _qara (generator_v3.py:48-173) for every env, in ONE
        launch, from the env's current state (after reset(), or wherever the last call left it): rounds of policy + step
        spliced into -> data, label int32 [num_envs, L], info.  datatype: "QA", "QAR" or "QARA"; the layouts and the
        reference behaviours kept are in metalang/stream_host.py.  An env stops when its data row is full or after
        max_rounds rounds (default ceil(L / the shortest round): always enough; fewer leave zeros behind info["filled"]).

        K = max_rounds x (2 for QARA, else 1) sub-steps (one policy + step pair each).  T_choices float64 [n]
        (default numpy.logspace(-1, 4, 20)); t_index int[num_envs, K]: the temperature of every sub-step as an index
        into T_choices (default: drawn from Philox).  draws: dict of float64 [num_envs, K, max_len + 1] for u_policy,
        u_greedy, u_low, u_query.  The call advances the tick by 2 K: sub-step k draws what policy() would at tick + 2 k
        and what step() would at tick + 2 k + 1, however many sub-steps an env needs.

        info: filled, rounds int32 [num_envs]; reward float64 and t_index int32 [num_envs, K] of the sub-steps that ran
        (0 and -1 elsewhere, and for QA, which forms no reward and answers at T = 1e-3)."""
        import torch
        from .stream_host import DATATYPES, SHORTEST_ROUND, default_T_choices, marks_of
        self._live()
        if datatype not in DATATYPES:
            raise ValueError("datatype must be one of QAR, QA, QARA")
        if int(L) != L or int(L) < 1:
            raise ValueError("L must be an integer of at least 1")
        L = int(L)
        if max_rounds is None:
            max_rounds = -(-L // SHORTEST_ROUND[datatype])
        if int(max_rounds) != max_rounds or int(max_rounds) < 1:
            raise ValueError("max_rounds must be an integer of at least 1")
        max_rounds = int(max_rounds)
        K = max_rounds * (2 if datatype == "QARA" else 1)
        choices = torch.as_tensor(default_T_choices() if T_choices is None else np.asarray(T_choices, np.float64),
                                  dtype=torch.float64).to(self.device).contiguous()
        if choices.dim() != 1 or choices.numel() < 1 or not bool(((choices > 0) & torch.isfinite(choices)).all()):
            raise ValueError("T_choices must be a non-empty 1-D array of positive finite temperatures")
        n_choice = int(choices.numel())
        ti = None
        if t_index is not None:
            if torch.is_tensor(t_index) and t_index.is_floating_point() or (
                    not torch.is_tensor(t_index) and np.asarray(t_index).dtype.kind not in "iu"):
                raise ValueError("t_index must be an integer array")
            ti = torch.as_tensor(t_index).to(self.device, torch.int32).contiguous()
            if tuple(ti.shape) != (self.num_envs, K):
                raise ValueError("t_index must have shape %s, got %s" % ((self.num_envs, K), tuple(ti.shape)))
            if datatype != "QA" and (int(ti.min()) < 0 or int(ti.max()) >= n_choice):
                raise ValueError("t_index must hold indices into the %d T_choices" % n_choice)
        us = []
        for key in ("u_policy", "u_greedy", "u_low", "u_query"):
            u = None
            if draws is not None and draws.get(key) is not None:
                u = torch.as_tensor(draws[key], dtype=torch.float64).to(self.device).contiguous()
                if tuple(u.shape) != (self.num_envs, K, self.max_len + 1):
                    raise ValueError("draws[%r] must have shape %s, got %s" % (key, (self.num_envs, K, self.max_len + 1),
                                                                               tuple(u.shape)))
            us.append(u)
        marks = (C.c_int32 * 11)(*marks_of())
        data = torch.empty((self.num_envs, L), dtype=torch.int32, device=self.device)
        label = torch.empty((self.num_envs, L), dtype=torch.int32, device=self.device)
        filled = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        rounds = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        reward = torch.zeros((self.num_envs, K), dtype=torch.float64, device=self.device)
        t_used = torch.full((self.num_envs, K), -1, dtype=torch.int32, device=self.device)
        code = DATATYPES.index(datatype)      # XV_METALM_QA, _QAR, _QARA
        _lib.check(self.lib.xv_metalm_stream(self._h, code, L, max_rounds, _lib.ptr(choices), n_choice, _lib.ptr(ti),
                                             *(_lib.ptr(u) for u in us), marks, _lib.ptr(data), _lib.ptr(label),
                                             _lib.ptr(filled), _lib.ptr(rounds), _lib.ptr(reward), _lib.ptr(t_used)))
        return data, label, dict(filled=filled, rounds=rounds, reward=reward, t_index=t_used)

    # ---- state ------------------------------------------------------------------------------------------------------
    def get_state(self):
        """what a later set_state needs to go on as if nothing had happened: the queries, the cached hidden states, the
        step counters and the engine's tick"""
        import torch
        self._live()
        query, query_len = self._tokens()
        cache = torch.empty((self.num_envs, self.n_hidden), dtype=torch.float64, device=self.device)
        steps = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.xv_metalm_get_state(self._h, _lib.ptr(query), _lib.ptr(query_len), _lib.ptr(cache),
                                                _lib.ptr(steps)))
        return dict(query=query, query_len=query_len, cache=cache, steps=steps, tick=self.engine.tick)

    def set_state(self, state):
        import torch
        self._live()
        t = [torch.as_tensor(state[k]).to(self.device, d).contiguous()
             for k, d in (("query", torch.int32), ("query_len", torch.int32), ("cache", torch.float64),
                          ("steps", torch.int32))]
        shapes = [(self.num_envs, self.max_len), (self.num_envs,), (self.num_envs, self.n_hidden), (self.num_envs,)]
        for x, s in zip(t, shapes):
            if tuple(x.shape) != s:
                raise ValueError("set_state: a tensor has shape %s, expected %s" % (tuple(x.shape), s))
        _lib.check(self.lib.xv_metalm_set_state(self._h, *(_lib.ptr(x) for x in t)))
        self.engine.tick = int(state["tick"])

    def check_errors(self, clear=True):
        """the engine's sticky device error word (0: none; include/xeno.h XV_DEVERR_*)"""
        return self.engine.error_flags(clear)

    def _destroy(self):
        if self._h is not None:
            self.lib.xv_metalm_destroy(self._h)
            self._h = None
            self._tables = None

    def close(self):
        self._destroy()
        if getattr(self, "engine", None) is not None:
            self.engine.close()
            self.engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MetaLMV3Env(object):
    """The reference's MetaLMV3Env (metalangv3.py:4-42) on a one-env batch.  As there: step's fourth return value is
    `steps < max_steps`, verbatim (MetaLMV3VecEnv returns truncated = steps >= max_steps), and step(cached=True) hands
    back the query of reset() while the language model keeps the state its last generated query left.  `seed` keys the
    Philox streams (the reference draws from numpy's global generator: other numbers, same distribution); draws= injects
    the uniforms of a call, as in MetaLMV3VecEnv, as 1-D arrays."""

    def __init__(self, max_steps=10000, device="cuda:0", max_len=1024, seed=0):
        from ..spaces import Discrete
        self.max_steps = max_steps
        self.device, self.max_len, self.seed = device, int(max_len), seed
        self.action_space = self.observation_space = Discrete(16)
        self.task_set = False
        self._vec = None

    def set_task(self, task):
        from ..spaces import Discrete
        lm = _lm_of(task, "task")
        self.vocabulary = task.get("vocabulary", lm.n_vocab)
        self.embedding = task.get("embedding", lm.n_emb)
        self.hidden = task.get("hidden", lm.n_hidden)
        self.function_vocabulary = task.get("function_vocabulary")
        self.lm = lm
        if self._vec is None:
            self._vec = MetaLMV3VecEnv(1, max_len=self.max_len, max_steps=self.max_steps, device=self.device, seed=self.seed)
        self._vec.set_task(dict(task, lm=lm))
        self.action_space = self.observation_space = Discrete(self.vocabulary)
        self.task_set = True

    def _draws(self, draws):
        if draws is None:
            return None
        out = {}
        for k, v in draws.items():
            row = np.full((1, self.max_len + 1), 0.5)
            v = np.asarray(v, np.float64).reshape(-1)
            row[0, :len(v)] = v
            out[k] = row
        return out

    @staticmethod
    def _row(tokens, length):
        return [int(t) for t in tokens[0, :int(length[0])].cpu().numpy()]

    def _flags(self):
        flags = self._vec.check_errors()
        if flags:
            raise _lib.XenoError("MetaLMV3Env: device error flags 0x%x (include/xeno.h XV_DEVERR_*)" % flags)

    def reset(self, *args, draws=None, **kwargs):
        if not self.task_set:
            raise Exception("Task not set")
        self.cached_query = self._row(*self._vec.reset(draws=self._draws(draws)))
        self._flags()
        self.steps = 0
        return self.cached_query

    def step(self, action, cached=False, draws=None):
        action = [int(a) for a in action]
        if len(action) > self.max_len:
            raise ValueError("an action of %d tokens is longer than max_len = %d" % (len(action), self.max_len))
        ans = np.zeros((1, self.max_len), np.int32)
        ans[0, :len(action)] = action
        obs, r, _, _, info = self._vec.step(ans, np.array([len(action)], np.int32), cached=bool(cached),
                                            draws=self._draws(draws))
        self._flags()
        s = self.cached_query if cached else self._row(*obs)
        self.steps += 1
        label = [int(t) for t in info["label"][0, :len(action) + 1].cpu().numpy()]
        return tuple(s), float(r[0]), False, (self.steps < self.max_steps), {"label": label}

    def policy(self, T=1.0, draws=None):
        if not self.task_set:
            raise Exception("Task not set")
        ans = self._row(*self._vec.policy(T, draws=self._draws(draws)))
        self._flags()
        return ans

    def close(self):
        if self._vec is not None:
            self._vec.close()
            self._vec = None
