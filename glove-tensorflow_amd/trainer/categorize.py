"""`python -m trainer.categorize --job-dir J --categories FILE [--embeddings row|col|sum] [--restrict-vocab N] [--no-lowercase]
[--delimiter D] [--word-column 1] [--category-column 2] [--clusters K] [--restarts 10] [--iterations 100] [--seed 0]`

Concept categorization (AP, BLESS, Battig, ESSLLI-2008; Baroni et al. 2014, Schnabel et al. 2015): the words of a
gold-labelled set are clustered by spherical k-means on the GPU (include/glove_eval_cluster_hip.h) against the newest
checkpoint of J, and the clusters' purity against the gold categories is the score.  The reference does not have this.
Writes J/eval/categorization.json.  One process, like trainer.analogy.

This module holds the file format and the purity; `Estimator.evaluate_categorization` does the work.
"""
from __future__ import annotations

import argparse
import json
import logging
from pathlib import Path

import numpy as np

from trainer import config
from trainer.analogy import EMBEDDINGS, SKIPPED_TOKEN

logger = logging.getLogger(__name__)


def parse_categories(path, lowercase=True, delimiter=None, word_column=1, category_column=2) -> list:
    """[(line number, word, category), ...] in file order.  One word per line, `word category` split on whitespace or on
    `delimiter`, the two in the columns `word_column` and `category_column` (counted from 1).  Blank lines and lines
    starting with `#` are skipped; a line with too few columns is an error that names it.  Words are lowercased unless
    told otherwise, category names are taken as written."""
    if word_column < 1 or category_column < 1 or word_column == category_column:
        raise ValueError("--word-column and --category-column must be two different columns counted from 1, got %r and %r"
                         % (word_column, category_column))
    need = max(word_column, category_column)
    rows = []
    with open(path, encoding="utf8") as f:
        for lineno, line in enumerate(f, 1):
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            fields = [x.strip() for x in line.rstrip("\r\n").split(delimiter)] if delimiter else line.split()
            if len(fields) < need or not fields[word_column - 1] or not fields[category_column - 1]:
                raise ValueError("%s line %d: expected at least %d columns, a word in column %d and a category in column %d"
                                 % (path, lineno, need, word_column, category_column))
            word = fields[word_column - 1]
            rows.append((lineno, word.lower() if lowercase else word, fields[category_column - 1]))
    return rows


def lookup_words(rows, vocab, limit=None):
    """Words -> ids under the rules of wordsim.lookup_pairs.  `vocab`: tokens in id order, used as they are; `limit`:
    ids from it on do not exist (--restrict-vocab).  Returns (ids of the words kept, in file order, their categories,
    the number of lines skipped, the number of duplicates).  A line is skipped when its word is missing, is "<UNK>", or
    lies at or beyond the limit; a word seen again keeps its first line, and the later ones count as duplicates."""
    ids_of = {}
    for i, token in enumerate(vocab):
        if token != SKIPPED_TOKEN and (limit is None or i < limit):
            ids_of.setdefault(token, i)
    ids, categories, seen, skipped, duplicates = [], [], set(), 0, 0
    for _, word, category in rows:
        i = ids_of.get(word)
        if i is None:
            skipped += 1
        elif i in seen:
            duplicates += 1
        else:
            seen.add(i)
            ids.append(i)
            categories.append(category)
    return ids, categories, skipped, duplicates


def purity(assign, categories):
    """(1 / n) sum over the clusters of the size of the cluster's largest gold category; None without words."""
    assign = np.asarray(assign).tolist()
    if len(assign) != len(categories):
        raise ValueError("purity: %d assignments and %d categories" % (len(assign), len(categories)))
    if not assign:
        return None
    table = {}
    for cluster, category in zip(assign, categories):
        per = table.setdefault(cluster, {})
        per[category] = per.get(category, 0) + 1
    return sum(max(per.values()) for per in table.values()) / len(assign)


def main(job_dir=config.JOB_DIR, categories=None, embeddings="row", restrict_vocab=None, no_lowercase=False, delimiter=None,
         word_column=1, category_column=2, clusters=None, restarts=10, iterations=100, seed=0, **_):
    from trainer.estimator import Estimator
    params = json.loads(Path(job_dir, "params.json").read_text())
    return Estimator(params).evaluate_categorization(
        categories, embeddings=embeddings, restrict_vocab=restrict_vocab, lowercase=not no_lowercase, delimiter=delimiter,
        word_column=word_column, category_column=category_column, clusters=clusters, restarts=restarts,
        iterations=iterations, seed=seed)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    cli.add_argument("--job-dir", default=config.JOB_DIR, help="job directory of a finished or running training")
    cli.add_argument("--categories", required=True, help="gold file: lines of `word category`; blank and # lines are skipped")
    cli.add_argument("--embeddings", choices=EMBEDDINGS, default="row", help="row table, col table, or their sum (the GloVe paper's W + W~)")
    cli.add_argument("--restrict-vocab", type=int, default=None, help="use the first N vocabulary rows only")
    cli.add_argument("--no-lowercase", action="store_true", help="take the words as written instead of lowercasing them")
    cli.add_argument("--delimiter", default=None, help="column separator (default: any whitespace)")
    cli.add_argument("--word-column", type=int, default=1, help="column of the word, counted from 1")
    cli.add_argument("--category-column", type=int, default=2, help="column of the gold category, counted from 1")
    cli.add_argument("--clusters", type=int, default=None, help="number of clusters (default: the gold categories among the words kept)")
    cli.add_argument("--restarts", type=int, default=10, help="k-means runs from different initial centroids; the best objective wins")
    cli.add_argument("--iterations", type=int, default=100, help="assign passes per run at the most")
    cli.add_argument("--seed", type=int, default=0, help="seed of the initial centroids")
    try:
        main(**vars(cli.parse_args()))
    except KeyboardInterrupt:
        pass
