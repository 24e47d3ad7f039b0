"""`python -m trainer.classes --job-dir J --classes K [--embeddings row|col|sum] [--restrict-vocab N] [--iterations 10]
[--restarts 1] [--seed 0]`

word2vec's `-classes K`: one class id per vocabulary word, by spherical k-means of the newest checkpoint's rows on the
GPU (include/glove_eval_cluster_hip.h).  Writes J/classes.txt — lines `token class` in vocabulary order, "<UNK>" left out
(it is not clustered either) — and J/eval/classes.json.  The reference does not have this.  One process.

`Estimator.word_classes` does the work.
"""
from __future__ import annotations

import argparse
import json
import logging
from pathlib import Path

from trainer import config
from trainer.analogy import EMBEDDINGS

logger = logging.getLogger(__name__)


def main(job_dir=config.JOB_DIR, classes=None, embeddings="row", restrict_vocab=None, iterations=10, restarts=1, seed=0, **_):
    from trainer.estimator import Estimator
    params = json.loads(Path(job_dir, "params.json").read_text())
    return Estimator(params).word_classes(classes, embeddings=embeddings, restrict_vocab=restrict_vocab,
                                          iterations=iterations, restarts=restarts, seed=seed)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    cli.add_argument("--job-dir", default=config.JOB_DIR, help="job directory of a finished or running training")
    cli.add_argument("--classes", type=int, required=True, help="number of word classes")
    cli.add_argument("--embeddings", choices=EMBEDDINGS, default="row", help="row table, col table, or their sum (the GloVe paper's W + W~)")
    cli.add_argument("--restrict-vocab", type=int, default=None, help="use the first N vocabulary rows only")
    cli.add_argument("--iterations", type=int, default=10, help="assign passes per run at the most (word2vec runs 10)")
    cli.add_argument("--restarts", type=int, default=1, help="k-means runs from different initial centroids; the best objective wins")
    cli.add_argument("--seed", type=int, default=0, help="seed of the initial centroids")
    try:
        main(**vars(cli.parse_args()))
    except KeyboardInterrupt:
        pass
