"""`python -m trainer.analogy --job-dir J --questions FILE [--embeddings row|col|sum] [--top-k 1] [--batch-size 1024]
[--restrict-vocab N] [--no-lowercase] [--method 3cosadd|3cosmul] [--epsilon 0.001]`

Scores the word-analogy questions `a : b :: c : ?` of a `questions-words.txt`-style file (`: section` lines, then lines of
four tokens) against the newest checkpoint of J: 3CosAdd on the GPU (include/glove_eval_hip.h), the stock intrinsic check
of GloVe and word2vec embeddings, which the reference does not have.  Writes J/eval/analogy.json.  One process: checkpoints
hold the whole model in vocabulary order however the run was sharded or relabelled.  `--method 3cosmul` scores by Levy &
Goldberg's 3CosMul instead (include/glove_eval_sim_hip.h) and writes J/eval/analogy_3cosmul.json.

This module holds the file format and the bookkeeping; `Estimator.evaluate_analogies` does the work.
"""
from __future__ import annotations

import argparse
import json
import logging
from pathlib import Path

from trainer import config

logger = logging.getLogger(__name__)
SKIPPED_TOKEN = "<UNK>"
EMBEDDINGS = ("row", "col", "sum")
METHODS = ("3cosadd", "3cosmul")
SYNTACTIC_PREFIX = "gram"       # word2vec's convention: sections named gram1-adjective-to-adverb, ... are syntactic


def parse_questions(path, lowercase=True) -> list:
    """[(section name, [(line number, (a, b, c, expected)), ...]), ...] in file order.  Questions in front of the first
    `: section` line go to a section with an empty name; a line that is not four tokens is an error that names it."""
    sections = []
    with open(path, encoding="utf8") as f:
        for lineno, line in enumerate(f, 1):
            tokens = line.split()
            if not tokens:
                continue
            if tokens[0].startswith(":"):
                sections.append((line.strip()[1:].strip(), []))
                continue
            if len(tokens) != 4:
                raise ValueError("%s line %d: expected four tokens, got %d" % (path, lineno, len(tokens)))
            if not sections:
                sections.append(("", []))
            sections[-1][1].append((lineno, tuple(t.lower() for t in tokens) if lowercase else tuple(tokens)))
    return sections


def lookup_questions(sections, vocab, limit=None):
    """Question words -> ids.  `vocab`: tokens in id order, used as they are; `limit`: ids from it on do not exist
    (--restrict-vocab).  Returns (ids [(a, b, c, expected), ...] of the questions kept, in order, and per section the
    pair (kept, skipped)).  A question is skipped when one of its four words is missing, is "<UNK>", or lies at or
    beyond the limit."""
    ids_of = {}
    for i, token in enumerate(vocab):
        if token != SKIPPED_TOKEN and (limit is None or i < limit):
            ids_of.setdefault(token, i)
    kept, counts = [], []
    for _, questions in sections:
        n = 0
        for _, words in questions:
            ids = [ids_of.get(w) for w in words]
            if any(i is None for i in ids):
                continue
            kept.append(tuple(ids))
            n += 1
        counts.append((n, len(questions) - n))
    return kept, counts


def tally(correct, total, skipped) -> dict:
    return {"correct": int(correct), "total": int(total), "skipped": int(skipped),
            "accuracy": correct / total if total else None}


def summarize(sections, counts, hits) -> dict:
    """The per-section and overall counts of analogy.json.  `hits`: one bool per kept question, in order."""
    out, pos = [], 0
    for (name, _), (n, skipped) in zip(sections, counts):
        out.append(dict(name=name, **tally(sum(bool(h) for h in hits[pos:pos + n]), n, skipped)))
        pos += n

    def merged(rows):
        return tally(sum(r["correct"] for r in rows), sum(r["total"] for r in rows), sum(r["skipped"] for r in rows))
    syntactic = [r for r in out if r["name"].startswith(SYNTACTIC_PREFIX)]
    semantic = [r for r in out if not r["name"].startswith(SYNTACTIC_PREFIX)]
    total = merged(out)
    return {"sections": out, "semantic": merged(semantic), "syntactic": merged(syntactic), "total": total,
            "questions_seen": total["total"], "questions_total": total["total"] + total["skipped"]}


def main(job_dir=config.JOB_DIR, questions=None, embeddings="row", top_k=1, batch_size=1024, restrict_vocab=None,
         no_lowercase=False, method="3cosadd", epsilon=1e-3, **_):
    from trainer.estimator import Estimator
    params = json.loads(Path(job_dir, "params.json").read_text())
    return Estimator(params).evaluate_analogies(questions, embeddings=embeddings, top_k=top_k, batch_size=batch_size,
                                                restrict_vocab=restrict_vocab, lowercase=not no_lowercase, method=method,
                                                epsilon=epsilon)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    cli.add_argument("--job-dir", default=config.JOB_DIR, help="job directory of a finished or running training")
    cli.add_argument("--questions", required=True, help="question file: `: section` lines, then lines of four tokens")
    cli.add_argument("--embeddings", choices=EMBEDDINGS, default="row", help="row table, col table, or their sum (the GloVe paper's W + W~)")
    cli.add_argument("--top-k", type=int, default=1, help="a question counts as correct if the expected word is among this many best")
    cli.add_argument("--batch-size", type=int, default=1024, help="questions per GPU call (their scores are a [batch, V] matrix)")
    cli.add_argument("--restrict-vocab", type=int, default=None, help="use the first N vocabulary rows only, as table and as candidates")
    cli.add_argument("--no-lowercase", action="store_true", help="take the question words as written instead of lowercasing them")
    cli.add_argument("--method", choices=METHODS, default="3cosadd", help="3cosadd: cos(b - a + c, v); 3cosmul: cos(b, v) cos(c, v) / (cos(a, v) + epsilon) on cosines shifted to [0, 1]")
    cli.add_argument("--epsilon", type=float, default=0.001, help="3cosmul's guard against a zero denominator, in (0, 1]: the paper's value (gensim uses 1e-6)")
    try:
        main(**vars(cli.parse_args()))
    except KeyboardInterrupt:
        pass
