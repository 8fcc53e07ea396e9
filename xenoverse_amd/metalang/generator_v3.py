"""python -m xenoverse_amd.metalang.generator_v3: the reference's MetaLMV3 data generator (xenoverse/metalang/generator_v3.py),
same functions, flags and file formats: a pickled list of accepted task dicts (--sample_type tasks), or per task one stream
of query / answer / reward tokens with its label stream (--sample_type sequences) as an .npy of [samples, 2, L] or as
tab-separated token lines.  Where the reference runs its env one call at a time, every task's stream is assembled on the
device in one launch (MetaLMV3VecEnv.stream, csrc/metalm.hip); the formats and the reference behaviours kept are stated in
metalang/stream_host.py."""
import argparse
import pickle
import random
import time

import numpy

from .device_sampler import sample_tasks_device, task_dicts_from_device
from .generator import _text_io
from .lm_host import TaskSamplerV3
from .stream_host import CHECK_T_HIGH, CHECK_T_LOW, accepts, sample_tasks_host

MAX_ENVS_PER_CALL = 4096


def _max_len(max_len):
    return 1024 if max_len is None else int(max_len)


def generate_data_v3_batch(tasks, datatype, L, T_choices=None, device="cuda:0", seed=0, max_len=None):
    """one stream per task -> int32 [len(tasks), 2, L]: [:, 0] data, [:, 1] label.  Every task gets an env of its own (all
    of one size); reset(), then one stream() launch per MAX_ENVS_PER_CALL tasks.  tasks: task dicts, or the tables dict of
    sample_tasks_device, whose device tensors are sliced per call and set as they are."""
    from .device_sampler import is_tables, slice_tables
    from .lm_env import MetaLMV3VecEnv
    tables = tasks if is_tables(tasks) else None
    tasks = None if tables is not None else list(tasks)
    n = int(tables["emb"].shape[0]) if tables is not None else len(tasks)
    out = numpy.zeros((n, 2, int(L)), numpy.int32)
    for base in range(0, n, MAX_ENVS_PER_CALL):
        top = min(n, base + MAX_ENVS_PER_CALL)
        part = slice_tables(tables, base, top) if tables is not None else tasks[base:top]
        env = MetaLMV3VecEnv(top - base, max_len=_max_len(max_len), device=device, seed=seed, env_id_base=base)
        try:
            env.set_task(part)
            env.reset()
            data, label, info = env.stream(datatype, L, T_choices=T_choices)
            out[base:top, 0] = data.cpu().numpy()
            out[base:top, 1] = label.cpu().numpy()
            flags = env.check_errors()
        finally:
            env.close()
        if flags:
            raise RuntimeError("device error flags 0x%x (include/xeno.h XV_DEVERR_*)" % flags)
    return out


def _single(task, datatype, T_choices, L):
    out = generate_data_v3_batch([task], datatype, L, T_choices=T_choices, seed=int(time.time() * 1000 % 1000000))
    return out[0, 0].copy(), out[0, 1].copy()


def generate_data_v3_single_task_qar(task, T_choices=None, L=10000):
    return _single(task, "QAR", T_choices, L)


def generate_data_v3_single_task_qara(task, T_choices=None, L=10000):
    return _single(task, "QARA", T_choices, L)


def generate_data_v3_single_task_qa(task, T_choices=None, L=10000):
    return _single(task, "QA", T_choices, L)


def _check_rewards_device(tasks, device, seed):
    """reset, policy(T=10000), step(cached), policy(T=1e-6), step(cached) for one env per task -> (reward_low, reward_high)"""
    from .lm_env import MetaLMV3VecEnv
    env = MetaLMV3VecEnv(len(tasks), device=device, seed=seed)
    try:
        env.set_task(tasks)
        env.reset()
        rewards = []
        for T in (CHECK_T_LOW, CHECK_T_HIGH):
            answer, answer_len = env.policy(T)
            rewards.append(env.step(answer, answer_len, cached=True)[1].cpu().numpy())
        env.check_errors()      # a pass cut at max_len still has a reward
    finally:
        env.close()
    return rewards[0], rewards[1]


def sample_and_check_tasks(n, vocab_size=32, embedding_size=16, hidden_size=32, function_token_number=6, seed=None,
                           backend="device", device="cuda:0"):
    """n tasks that the reference's sample_and_check_task would accept: after reset(), the reward of an answer at T = 10000
    is <= 0 and that of an answer at T = 1e-6 is >= 2.  Candidates are TaskSamplerV3(seed + j), j = 0, 1, ...; an attempt
    tests as many candidates as tasks are still missing, as one batch (the existing reset / policy / step calls).

    The reference passes the same seed to every attempt, so a seeded task that fails is retried forever; here the seed
    ADVANCES past a rejected candidate.  seed=None takes a base from the clock.  backend="host" runs the same test over
    RandomLMHost, one candidate at a time, without a GPU.  -> (tasks, the seeds they were made from)"""
    if seed is None:
        seed = int(time.time() * 1000 % 1000000)
    seed = int(seed)
    if backend == "host":
        return sample_tasks_host(n, vocab_size, embedding_size, hidden_size, seed)
    if backend != "device":
        raise ValueError("backend must be 'device' or 'host'")
    tasks, seeds = [], []
    while len(tasks) < n:
        batch = n - len(tasks)
        cand = [TaskSamplerV3(vocab_size, embedding_size, hidden_size, seed=seed + j) for j in range(batch)]
        low, high = _check_rewards_device(cand, device, seed)
        for j in range(batch):
            if accepts(float(low[j]), float(high[j])):
                tasks.append(cand[j])
                seeds.append(seed + j)
        seed += batch
    return tasks, seeds


def sample_and_check_task(vocab_size=32, embedding_size=16, hidden_size=32, function_token_number=6, seed=None,
                          backend="device", device="cuda:0"):
    """the reference's signature -> one accepted task (see sample_and_check_tasks: a seed that fails advances)"""
    return sample_and_check_tasks(1, vocab_size, embedding_size, hidden_size, function_token_number, seed, backend,
                                  device)[0][0]


def _sample_tables(samples, seed, device, sizes):
    return sample_tasks_device(samples, sizes["vocab_size"], sizes["embedding_size"], sizes["hidden_size"], seed=seed,
                               device=device)


def metalang_generator_v3(datatype="QAR", sample_type="sequences", vocab_size=32, embedding_size=16, hidden_size=32,
                          samples=1000, sequence_length=16000, output_type="txt", task_file=None, output=None,
                          device="cuda:0", seed=None, backend="device", sampler=None):
    """sampler: None — tasks come from sample_and_check_tasks(backend=backend), as ever; "device" — from
    sample_tasks_device: made and tested on the GPU, handed to the streams as device tables (other tasks than the former's
    for the same seed; they are drawn independently, so they are not shuffled)"""
    seed_base = int(time.time() * 1000 % 1000000) if seed is None else int(seed)
    assert datatype in ["QAR", "QA", "QARA"], "datatype must be one of QAR, QA, QARA"
    sizes = dict(vocab_size=vocab_size, embedding_size=embedding_size, hidden_size=hidden_size, function_token_number=6)
    if sample_type == "tasks":
        if output is None:
            raise Exception("Must specify --output when sample_type is tasks")
        if sampler == "device":
            tasks = task_dicts_from_device(_sample_tables(samples, seed_base, device, sizes))
        else:
            tasks, _ = sample_and_check_tasks(samples, seed=seed_base, backend=backend, device=device, **sizes)
        name = output if output.endswith(".pkl") else output + ".pkl"
        with open(name, "wb") as f:
            pickle.dump(tasks, f)
        return None
    if task_file is None and sampler == "device":
        tasks = _sample_tables(samples, seed_base, device, sizes)
        if backend == "host":
            tasks = task_dicts_from_device(tasks)
    else:
        if task_file is None:      # a task of its own for every sample
            tasks, _ = sample_and_check_tasks(samples, seed=seed_base, backend=backend, device=device, **sizes)
        else:
            with open(task_file, "rb") as f:
                tasks = pickle.load(f)
        random.Random(seed_base).shuffle(tasks)
    if backend == "host":
        from .stream_host import generate_data_v3_host
        data = numpy.array([generate_data_v3_host(t, datatype, sequence_length)[:2] for t in tasks])
    else:
        data = generate_data_v3_batch(tasks, datatype, sequence_length, device=device, seed=seed_base)
    print(data.shape)
    if output_type == "npy":
        numpy.save(output, data)
    elif output_type == "txt":
        _text_io(data, output)
    return data


def main(argv=None):
    ap = argparse.ArgumentParser(description="Generating Meta Language Tasks or Sequences (MetaLMV3, on the GPU)")
    ap.add_argument("--sample_type", type=str, choices=["tasks", "sequences"], default="sequences",
                    help="Generate tasks or sequences")
    ap.add_argument("--datatype", type=str, choices=["QAR", "QA", "QARA"], default="QAR",
                    help="Query-Answer, Query-Answer-Reward, or Query-Answer-Reward-Answer")
    ap.add_argument("--task_file", type=str, default=None,
                    help="task file to generate from if the sample_type is sequences; default: tasks on the fly")
    ap.add_argument("--vocab_size", type=int, default=32)
    ap.add_argument("--embedding_size", type=int, default=16)
    ap.add_argument("--hidden_size", type=int, default=32)
    ap.add_argument("--sequence_length", type=int, default=16000)
    ap.add_argument("--samples", type=int, default=10, help="number of sequences / tasks to generate")
    ap.add_argument("--output_type", type=str, choices=["txt", "npy"], default="txt")
    ap.add_argument("--output", type=str, default=None)
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--seed", type=int, default=None, help="task seeds and the Philox key; default: from the clock, as the reference")
    ap.add_argument("--backend", type=str, choices=["device", "host"], default="device",
                    help="host: the numpy restatement, no GPU (slow; for checking)")
    ap.add_argument("--sampler", type=str, choices=["device"], default=None,
                    help="device: make and test the tasks on the GPU in one launch per batch (metalang.sample_tasks_device)")
    metalang_generator_v3(**vars(ap.parse_args(argv)))


if __name__ == "__main__":
    main()
