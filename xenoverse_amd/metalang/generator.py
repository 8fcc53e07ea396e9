"""python -m xenoverse_amd.metalang.generator: the reference's generator CLI (xenoverse/metalang/generator.py) for
--version v2, same flags and file formats: a pickled list of task dicts (--sample_type tasks), tab-separated token lines or
one .npy (--sample_type sequences).  Where the reference generates one task at a time, the groups of all tasks go to the
device in one call.  --sample_type tasks needs no GPU."""
import argparse
import pickle
import random
import sys
import time

import numpy

from .task_sampler import TaskSamplerV2


def _text_io(tokens, output):
    stream = open(output, "w") if isinstance(output, str) else sys.stdout
    for row in tokens:
        stream.write("\t".join(map(str, row.tolist())))
        stream.write("\n")
    if isinstance(output, str):
        stream.close()


def _sample_tasks(samples, seed_base, vocab_size, embedding_size, hidden_size, n_gram, lambda_weight):
    n_gram = list(n_gram) if isinstance(n_gram, (list, tuple)) else n_gram
    return [TaskSamplerV2(seed=i + seed_base, n_vocab=vocab_size, n_emb=embedding_size, n_hidden=hidden_size,
                          n_gram=n_gram, _lambda=lambda_weight) for i in range(samples)]


def _sample_tables(samples, seed_base, device, vocab_size, embedding_size, hidden_size, n_gram, lambda_weight):
    from .device_sampler_v2 import sample_tasks_v2_device
    n_gram = list(n_gram) if isinstance(n_gram, (list, tuple)) else n_gram
    return sample_tasks_v2_device(samples, n_emb=embedding_size, n_hidden=hidden_size, n_vocab=vocab_size, n_gram=n_gram,
                                  _lambda=lambda_weight, seed=seed_base, device=device)


def metalang_generator(sample_type="sequences", version="v2", vocab_size=64, n_gram=3, embedding_size=16, hidden_size=64,
                       samples=1000, lambda_weight=5.0, batch_size=1, task_file=None, sequence_length=4096,
                       output_type="txt", output=None, device="cuda:0", seed=None, sampler=None):
    """sampler: None — tasks come from TaskSamplerV2 on numpy's stream, seeds seed .. seed + samples - 1, as ever; "device" —
    from sample_tasks_v2_device(seed=seed): made on the GPU and handed to the generator as device tables (other tasks than
    the former's for the same seed; they are drawn independently, so they are not shuffled)"""
    if version != "v2":
        raise SystemExit("MetaLang%s is not provided by xenoverse_amd (only --version v2 is; DESIGN.md §6)" % version.upper())
    seed_base = int(time.time() * 1000 % 1000000) if seed is None else int(seed)
    sizes = dict(vocab_size=vocab_size, embedding_size=embedding_size, hidden_size=hidden_size, n_gram=n_gram,
                 lambda_weight=lambda_weight)
    if sample_type == "tasks":
        if output is None:
            raise Exception("Must specify --output when sample_type is tasks")
        name = output if output.endswith(".pkl") else output + ".pkl"
        if sampler == "device":
            from .device_sampler_v2 import task_dicts_from_device_v2
            tasks = task_dicts_from_device_v2(_sample_tables(samples, seed_base, device, **sizes))
        else:
            tasks = _sample_tasks(samples, seed_base, **sizes)
        with open(name, "wb") as f:
            pickle.dump(tasks, f)
        return None
    from .batch import MetaLangV2Batch
    if task_file is None:       # a task of its own for every sample
        batch_size = 1
        tasks = _sample_tables(samples, seed_base, device, **sizes) if sampler == "device" else \
            _sample_tasks(samples, seed_base, **sizes)
    else:
        with open(task_file, "rb") as f:
            tasks = pickle.load(f)
    n_group = (samples - 1) // batch_size + 1
    if isinstance(tasks, list):
        if len(tasks) < n_group:
            tasks = tasks * ((n_group - 1) // len(tasks) + 1)
        random.Random(seed_base).shuffle(tasks)
        tasks = tasks[:n_group]
    gen = MetaLangV2Batch(n_group, batch_size, device=device, seed=seed_base)
    gen.set_task(tasks)
    tokens = gen.generate(sequence_length).reshape(n_group * batch_size, sequence_length + 1).cpu().numpy()
    flags = gen.check_errors()
    gen.close()
    if flags:
        raise RuntimeError("device error flags 0x%x" % flags)
    if output_type == "npy":
        numpy.save(output, tokens)
    else:
        _text_io(tokens, output)
    return tokens


def main(argv=None):
    ap = argparse.ArgumentParser(description="Generating Meta Language Tasks or Sequences (MetaLangV2, on the GPU)")
    ap.add_argument("--version", type=str, choices=["v1", "v2"], default="v2")
    ap.add_argument("--sample_type", type=str, choices=["tasks", "sequences"], default="sequences",
                    help="Generate tasks or sequences")
    ap.add_argument("--task_file", type=str, default=None,
                    help="task file to generate from if the sample_type is sequences; default: a task per sample")
    ap.add_argument("--vocab_size", type=int, default=64)
    ap.add_argument("--embedding_size", type=int, default=16)
    ap.add_argument("--hidden_size", type=int, default=16)
    ap.add_argument("--patterns_number", type=int, default=10, help="MetaLangV1 only: not used")
    ap.add_argument("--error_rate", type=float, default=0.20, help="MetaLangV1 only: not used")
    ap.add_argument("--n_gram", nargs="+", type=int, default=[3, 4, 5, 6], help="a [list of] length n used for generating tasks")
    ap.add_argument("--lambda_weight", type=float, default=5.0, help="lambda multiplied for softmax sampling")
    ap.add_argument("--batch_size", type=int, default=1)
    ap.add_argument("--sequence_length", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=100, help="number of sequences / tasks to generate")
    ap.add_argument("--output_type", type=str, choices=["txt", "npy"], default="txt")
    ap.add_argument("--output", type=str, default=None)
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--seed", type=int, default=None, help="task seeds and the Philox key; default: from the clock, as the reference")
    ap.add_argument("--sampler", type=str, choices=["device"], default=None,
                    help="device: make the tasks on the GPU in one launch (metalang.sample_tasks_v2_device)")
    args = vars(ap.parse_args(argv))
    for k in ("patterns_number", "error_rate"):
        args.pop(k)
    metalang_generator(**args)


if __name__ == "__main__":
    main()
