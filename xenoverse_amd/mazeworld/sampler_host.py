"""Host restatement (numpy) of the device MazeWorld task sampler and resampler (csrc/maze_sampler.hip:
xv_maze_sample_tasks, xv_maze_resample_tasks): the same Philox counters, the same draw constructions and the same
arithmetic in the same order.  It is what the device is compared with, bit for bit (tests/test_gpu_maze_sampler.py), as
linds/sampler_host.py is for the LinDS sampler.

Counter layout (include/xeno.h): key = seed; counter = {index lo, index hi, sub, purpose | tick << 8}.  `index` is the
candidate (sampler) or the task index (resampler), `tick` the pass of the wall release (sampler) or the episode
(resampler), below 2^24.  One call gives two uniforms: words 0,1 and words 2,3 by xv_u53.  Element q of a block of
uniforms is half q & 1 of call sub = q >> 1.  Integers are floor(u * m).

The wall release (`genmaze_host`) is the parallel form of task_sampler.genmaze: per pass every standing interior wall is
tested on the grid as the pass found it, with its own key and its own P3 uniform; the passing wall with the smallest
(key, cell) is the one a walk in key order would stop at, the wall with the largest (key, cell) is where it would end
otherwise (`pass_tests`, `pass_choice`; tests/test_host_maze_sampler.py walks the same pass sequentially).
"""
import numpy as np

from ..host_draws import Draws, floor_int, interleave, uniform
from .tables import LMAX, NG_MAX
from .task_sampler import PI

STATUS = ("accepted", "pass_cap", "no_room")
N_MIN, N_MAX = 7, NG_MAX - 1
CMD_MAX = 2048
TICK_MAX = 1 << 24

# purposes (low byte of counter word 3); the resampler's are the sampler's | P_RESAMPLE
P_HEAD, P_ROOM, P_PASS, P_TEXT, P_LANDMARK, P_START, P_CMD, P_SHUFFLE, P_RESAMPLE = 0, 1, 2, 3, 4, 5, 6, 7, 0x10
# P_HEAD subs: 0 (cell_size, wall_height), 1 (agent_height, wall_density), 2 (landmarks_number, n),
#              3 (ground_text, ceiling_text), 4 (fol_angle, room count)
# P_ROOM sub 2 * (5 * room + try): (h, w); + 1: first half picks the placement
# P_PASS tick = pass, sub = cell: first half the key (its 53-bit integer), second half P3's uniform
# P_TEXT / P_LANDMARK / P_START / P_SHUFFLE: blocks of uniforms over cells (landmarks for P_SHUFFLE)
# P_CMD sub = i: first half command i, second half its fix-up
ROOM_TRIES = 5
INFO_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("rooms", "<i4"), ("passes", "<i4"), ("idle", "<i4"),
                       ("released", "<i4")])      # xv_maze_cand_info

DEFAULTS = dict(n_range=(9, 25), allow_loops=True, cell_size_range=(1.5, 4.5), wall_height_range=(2.0, 6.0),
                agent_height_range=(1.6, 2.0), wall_density_range=(0.2, 0.4), landmarks_number_range=(5, 15),
                fol_angle_range=(0.3 * PI, 0.8 * PI), commands_sequence=200, step_reward=0.0, collision_reward=-0.20,
                goal_reward=None, n_wall_textures=None, n_ground_textures=None, n_ceiling_textures=None)


def sampler_arguments(**kwargs):
    """MazeTaskSampler's keyword arguments (seed and verbose aside) with its defaults filled in and checked"""
    from .textures import REFERENCE_TEXTURE_COUNTS
    kwargs.pop("verbose", None)
    unknown = set(kwargs) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown sampler arguments: %s" % sorted(unknown))
    a = dict(DEFAULTS, **kwargs)
    for k, v in zip(("n_wall_textures", "n_ground_textures", "n_ceiling_textures"), REFERENCE_TEXTURE_COUNTS):
        a[k] = int(v if a[k] is None else a[k])
    n_lo, n_hi = int(a["n_range"][0]), int(a["n_range"][1])
    if not (N_MIN <= n_lo < n_hi and grid_pitch((n_lo, n_hi)) <= N_MAX):
        raise ValueError("n_range must give odd sizes within %d .. %d" % (N_MIN, N_MAX))
    if not (2 <= int(a["landmarks_number_range"][0]) < int(a["landmarks_number_range"][1])):
        raise ValueError("landmarks_number_range must start at 2 or above and be non-empty")
    if not (1 <= int(a["commands_sequence"]) <= CMD_MAX):
        raise ValueError("commands_sequence must be within 1 .. %d" % CMD_MAX)
    if min(a["n_wall_textures"], a["n_ground_textures"], a["n_ceiling_textures"]) < 1:
        raise ValueError("texture counts must be positive")
    return a


def grid_pitch(n_range):
    """NG: the largest n that n_range can give (randint's upper end is exclusive; even values are raised to odd)"""
    return (int(n_range[1]) - 1) | 1


def _randint(u, lo, hi):
    return int(lo) + int(floor_int(u, int(hi) - int(lo)))


# ---- rooms -------------------------------------------------------------------------------------------------------
def dig_rooms_host(d, n, n_rooms):
    """_dig_rooms under the sampler's draws -> (occ int8[n, n] with the border 0, walls int8[n, n], rooms)"""
    m = n - 2
    occ = np.zeros((n, n), np.int8)
    walls = np.ones((n, n), np.int8)
    rooms = []
    for r in range(n_rooms):
        for t in range(ROOM_TRIES):
            (uh, uk), (uw, _) = d.pairs(P_ROOM, [2 * (ROOM_TRIES * r + t), 2 * (ROOM_TRIES * r + t) + 1])
            h, w = 2 + int(floor_int(uh, 3)), 2 + int(floor_int(uw, 3))
            inner = occ[1:n - 1, 1:n - 1].astype(np.int64)
            c = np.cumsum(np.cumsum(np.pad(inner, ((1, 0), (1, 0))), 0), 1)
            win = c[h:, w:] - c[:-h, w:] - c[h:, :-w] + c[:-h, :-w]
            rows, cols = np.where(win == 0)
            if rows.shape[0] == 0:
                continue
            k = int(floor_int(uk, rows.shape[0]))
            r0, c0 = int(rows[k]), int(cols[k])
            occ[1 + max(0, r0 - 1):1 + min(m, r0 + h + 1), 1 + max(0, c0 - 1):1 + min(m, c0 + w + 1)] = 1
            walls[1 + r0:1 + r0 + h, 1 + c0:1 + c0 + w] = 0
            rooms.append((r0, c0, r0 + h - 1, c0 + w - 1))
            break
    return occ, walls, rooms


# ---- one pass of the wall release ----------------------------------------------------------------------------------
def pass_tests(walls, region, allow_loops, n_regions, u3):
    """Every interior cell tested as the pass finds the grid -> dict of [n-2, n-2] arrays: standing (an interior wall),
    passing (P1 | P2 | P3), ids int64[4, ...] (the open neighbours' region ids, -1 where closed; up, down, left, right),
    distinct, most, keep (the smallest neighbouring id, -1 without an open neighbour)."""
    n = walls.shape[0]
    nb = [(slice(0, n - 2), slice(1, n - 1)), (slice(2, n), slice(1, n - 1)),
          (slice(1, n - 1), slice(0, n - 2)), (slice(1, n - 1), slice(2, n))]
    ids = np.stack([np.where(walls[s] < 1, region[s].astype(np.int64), -1) for s in nb])
    distinct = np.zeros(ids.shape[1:], np.int64)
    most = np.ones(ids.shape[1:], np.int64)
    for t in range(4):
        first = ids[t] >= 0
        for s in range(t):
            first &= ids[s] != ids[t]
        distinct += first
        most = np.maximum(most, np.where(ids[t] >= 0, (ids == ids[t]).sum(0), 0))
    keep = np.where(ids < 0, np.iinfo(np.int64).max, ids).min(0)
    keep = np.where((ids >= 0).any(0), keep, -1)
    standing = walls[1:n - 1, 1:n - 1] > 0
    joins = distinct >= 2
    passing = joins & ((most < 2) | bool(allow_loops))
    if allow_loops and n_regions < 2:
        passing = passing | (u3 < 0.2)
    return dict(standing=standing, passing=passing & standing, ids=ids, distinct=distinct, most=most, keep=keep)


def pass_choice(tests, keys):
    """The wall the pass ends on, as interior (row, col), or None when no wall stands: the passing wall with the smallest
    (key, cell), else the standing wall with the largest (key, cell).  keys uint64[n-2, n-2]."""
    standing, passing = tests["standing"], tests["passing"]
    if not standing.any():
        return None
    flat = np.arange(standing.size).reshape(standing.shape)      # row-major: the order of the full grid's flat index
    if passing.any():
        cand = np.nonzero(passing.ravel())[0]
        order = np.lexsort((flat.ravel()[cand], keys.ravel()[cand]))
        pick = cand[order[0]]
    else:
        cand = np.nonzero(standing.ravel())[0]
        order = np.lexsort((flat.ravel()[cand], keys.ravel()[cand]))
        pick = cand[order[-1]]
    return int(pick // standing.shape[1]), int(pick % standing.shape[1])


def pass_draws(d, n, p):
    """keys uint64[n-2, n-2] and P3 uniforms float64[n-2, n-2] of pass p (sub = the cell's flat index in the n x n grid)"""
    i, j = np.meshgrid(np.arange(1, n - 1), np.arange(1, n - 1), indexing="ij")
    ka, kb = d.ints53(P_PASS, i * n + j, tick=p)
    return ka, kb.astype(np.float64) * (1.0 / 9007199254740992.0)


def genmaze_host(d, n, allow_loops, wall_density, on_pass=None):
    """-> (walls int8[n, n] or None at the pass cap, info dict).  on_pass(state dict) sees every pass before it acts."""
    m = n - 2
    n_rooms = _randint(d.pairs(P_HEAD, 4)[1], 0, m * m // 16)
    occ, walls, rooms = dig_rooms_host(d, n, n_rooms)
    region = np.full((n, n), -1, np.int64)
    for i in range(1, n, 2):
        for j in range(1, n, 2):
            if not occ[i, j]:
                walls[i, j] = 0
                region[i, j] = i * n + j
    n_regions = int((region >= 0).sum()) + len(rooms)
    for q, (r0, c0, r1, c1) in enumerate(rooms):
        region[r0 + 1:r1 + 2, c0 + 1:c1 + 2] = n * n + q
    n_walls = int(walls[1:-1, 1:-1].sum())
    budget = m * m * float(wall_density)
    cap = 4 * m * m
    passes = idle = released = 0
    while passes < cap and (n_regions > 1 or (allow_loops and n_walls > budget)):
        keys, u3 = pass_draws(d, n, passes)
        tests = pass_tests(walls, region, allow_loops, n_regions, u3)
        pick = pass_choice(tests, keys)
        if on_pass is not None:
            on_pass(dict(walls=walls.copy(), region=region.copy(), n_regions=n_regions, keys=keys, u3=u3, tests=tests,
                         pick=pick, index=passes))
        passes += 1
        if pick is None or tests["keep"][pick] < 0:
            idle += 1
            continue
        keep = int(tests["keep"][pick])
        ids = tests["ids"][(slice(None),) + pick]
        i, j = pick[0] + 1, pick[1] + 1
        walls[i, j] = 0
        region[i, j] = keep
        n_walls -= 1
        released += 1
        n_regions -= int(tests["distinct"][pick]) - 1
        for rid in ids:
            if rid >= 0 and rid != keep:
                region[(region == rid) & (walls < 1)] = keep
    done = not (n_regions > 1 or (allow_loops and n_walls > budget))
    info = dict(rooms=len(rooms), passes=passes, idle=idle, released=released)
    return (walls if done else None), info


# ---- landmarks, start, commands (shared with the resampler) ---------------------------------------------------------
def targets_host(d, walls, k, purpose=P_LANDMARK, tick=0):
    """_targets: like = u - walls; the k largest are the landmarks in ascending order of like (ties: the lower index
    ranks higher) -> (landmarks [(i, j)] * k, cell_landmarks int8[n, n])"""
    n = walls.shape[0]
    like = d.block(purpose, n * n, tick) - walls.reshape(-1).astype(np.float64)
    order = np.lexsort((np.arange(n * n), -like))[:k]       # descending like, lower index first
    idx = order[::-1]
    landmarks = [(int(c // n), int(c % n)) for c in idx]
    cl = np.full((n, n), -1, np.int8)
    for q, c in enumerate(landmarks):
        cl[c] = q
    return landmarks, cl


def start_host(d, walls, cell_landmarks, purpose=P_START, tick=0):
    """_start: the argmax of u - walls - cell_landmarks (ties: the lower index)"""
    n = walls.shape[0]
    like = d.block(purpose, n * n, tick) - walls.reshape(-1).astype(np.float64) - \
        cell_landmarks.reshape(-1).astype(np.float64)
    c = int(np.lexsort((np.arange(n * n), -like))[0])
    return (c // n, c % n)


def commands_host(d, k, length, purpose=P_CMD, tick=0):
    """_sample_cmds: `length` draws below k, immediate repeats moved on by 1 + floor(u * (k - 1)), left to right"""
    ua, ub = d.pairs(purpose, np.arange(length), tick)
    xs = floor_int(ua, k)
    step = 1 + floor_int(ub, k - 1)
    for i in range(1, length):
        if xs[i] == xs[i - 1]:
            xs[i] = (xs[i] + step[i]) % k
    return xs


# ---- the sampler ----------------------------------------------------------------------------------------------------
def sample_candidate_host(seed, cand, on_pass=None, **kwargs):
    """Candidate `cand` of `seed` -> (task dict in the reference's schema, or None when not accepted; info dict with
    status, n, rooms, passes, idle, released).  Keyword arguments: MazeTaskSampler's."""
    a = sampler_arguments(**kwargs)
    d = Draws(seed, cand)
    (u_cs, u_ah, u_lm, u_gt, u_fa), (u_wh, u_wd, u_n, u_ct, _) = d.pairs(P_HEAD, np.arange(5))
    cell_size = uniform(u_cs, *a["cell_size_range"])
    wall_height = uniform(u_wh, *a["wall_height_range"])
    agent_height = uniform(u_ah, *a["agent_height_range"])
    wall_density = uniform(u_wd, *a["wall_density_range"])
    k = min(_randint(u_lm, *a["landmarks_number_range"]), LMAX)
    n = _randint(u_n, *a["n_range"])
    if n % 2 == 0:
        n += 1
    ground_text = _randint(u_gt, 0, a["n_ground_textures"])
    ceiling_text = _randint(u_ct, 0, a["n_ceiling_textures"])
    fol_angle = uniform(u_fa, *a["fol_angle_range"])
    walls, info = genmaze_host(d, n, bool(a["allow_loops"]), wall_density, on_pass=on_pass)
    info = dict(info, n=n, status=0)
    if walls is None:
        return None, dict(info, status=1)
    if int((walls < 1).sum()) < k + 1:
        return None, dict(info, status=2)
    texts = floor_int(d.block(P_TEXT, n * n), a["n_wall_textures"]).reshape(n, n)
    inner = np.zeros((n, n), bool)
    inner[1:-1, 1:-1] = True
    texts[inner & (walls < 1)] = 0
    landmarks, cell_landmarks = targets_host(d, walls, k)
    start = start_host(d, walls, cell_landmarks)
    goal = n * np.sqrt(float(n)) / 60.0 if a["goal_reward"] is None else float(a["goal_reward"])
    task = {"start": start, "cell_walls": walls, "cell_texts": texts, "cell_size": float(cell_size),
            "ground_text": ground_text, "ceiling_text": ceiling_text, "step_reward": float(a["step_reward"]),
            "goal_reward": float(goal), "collision_reward": float(a["collision_reward"]),
            "wall_height": float(wall_height), "agent_height": float(agent_height), "fol_angle": float(fol_angle),
            "commands_sequence": commands_host(d, k, int(a["commands_sequence"])),
            "landmarks_coordinates": landmarks, "cell_landmarks": cell_landmarks}
    return task, info


def info_record(info):
    r = np.zeros((), INFO_DTYPE)
    for f in INFO_DTYPE.names:
        r[f] = info[f]
    return r


def sample_slots_host(seed, cand_base, n_cand, **kwargs):
    """Candidates [cand_base, cand_base + n_cand) as `device_sampler.sample_candidates` returns them, in numpy: the seven
    slots at pitch NG = grid_pitch(n_range) (all padding where status != 0), status, info records."""
    a = sampler_arguments(**kwargs)
    NG, n_cmd = grid_pitch(a["n_range"]), int(a["commands_sequence"])
    out = dict(NG=NG, n_cmd=n_cmd, walls=np.ones((n_cand, NG, NG), np.int8), texts=np.zeros((n_cand, NG, NG), np.int32),
               landmarks=np.full((n_cand, NG, NG), -1, np.int8), ints=np.zeros((n_cand, 8), np.int32),
               dbl=np.zeros((n_cand, 8), np.float64), commands=np.zeros((n_cand, n_cmd), np.int32),
               lm_coord=np.zeros((n_cand, LMAX, 2), np.int32), status=np.zeros(n_cand, np.int32),
               info=np.zeros(n_cand, INFO_DTYPE))
    from .tables import build_tables
    for q in range(n_cand):
        task, info = sample_candidate_host(seed, cand_base + q, **kwargs)
        out["info"][q] = info_record(info)
        out["status"][q] = info["status"]
        if task is None:
            continue
        t = build_tables([task])
        n = info["n"]
        for k in ("walls", "texts", "landmarks"):
            out[k][q, :n, :n] = t[k][0]
        for k in ("ints", "dbl", "commands", "lm_coord"):
            out[k][q] = t[k][0]
    return out


def slots_digest(slots, q):
    """candidate q's seven slots as one SHA-256 (uint8[32]), dbl[7] (the host's tan) left out: what
    tests/golden/sampler_maze_host_*.npz record of the batches whose numpy restatement takes minutes"""
    import hashlib
    h = hashlib.sha256()
    for k in ("walls", "texts", "landmarks", "ints", "dbl", "commands", "lm_coord"):
        v = np.ascontiguousarray(slots[k][q])
        h.update((v[:7] if k == "dbl" else v).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def resample_host(task, seed, index, episode, resample_cmd=True, resample_start=True, resample_landmarks=False,
                  resample_landmarks_color=False):
    """Resampler under the device's draws, a function of (seed, index, episode): keeps the scenario, re-draws landmarks
    (or permutes their colours by key rank), start and commands as the flags say."""
    if not 0 <= int(episode) < TICK_MAX:
        raise ValueError("episode must be within 0 .. 2^24 - 1")
    d = Draws(seed, index)
    new = dict(task)
    walls = np.asarray(task["cell_walls"], np.int8)
    k = len(task["landmarks_coordinates"])
    if resample_landmarks:
        landmarks, cl = targets_host(d, walls, k, P_LANDMARK | P_RESAMPLE, episode)
    elif resample_landmarks_color:
        keys = interleave(np.arange(k), *d.ints53(P_SHUFFLE | P_RESAMPLE, np.arange(k) >> 1, episode))
        order = np.lexsort((np.arange(k), keys))          # new landmark r is the old landmark order[r]
        landmarks = [tuple(int(v) for v in task["landmarks_coordinates"][q]) for q in order]
        cl = np.full_like(np.asarray(task["cell_landmarks"], np.int8), -1)
        for q, c in enumerate(landmarks):
            cl[c] = q
    else:
        landmarks = [tuple(int(v) for v in c) for c in task["landmarks_coordinates"]]
        cl = np.array(task["cell_landmarks"], np.int8)
    new["landmarks_coordinates"], new["cell_landmarks"] = landmarks, cl
    if resample_start:
        new["start"] = start_host(d, walls, cl, P_START | P_RESAMPLE, episode)
    if resample_cmd:
        new["commands_sequence"] = commands_host(d, k, len(task["commands_sequence"]), P_CMD | P_RESAMPLE, episode)
    return new
