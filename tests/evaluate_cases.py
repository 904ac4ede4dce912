"""What the evaluate tests share (and tests/golden/make_evaluate_golden.py builds its inputs from): synthetic call_mods result
rows, the goldens, one route run to (file bytes, stdout), and the gpu route's engine calls on top of the CPU checker."""
import json
import os

import numpy as np

from deepsignal_amd import engine as eng
from deepsignal_amd import evaluate_mods_call as ev

from table_backend import RememberedBatches

HERE = os.path.dirname(os.path.abspath(__file__))
KMER = "ACGTACGTCGACGTACG"
SUBSAMPLE_SEED = 7                                   # random.seed of the reference run, --seed of ours


def call_row(r, p1_text, label=None, p0_text=None, sep="\t"):
    """One call_mods result row around prob_1 = p1_text: prob_0 its complement at the same number of places, label 1 where
    prob_1 > prob_0 (unless given)."""
    places = len(p1_text.split(".")[1]) if "." in p1_text else 0
    if p0_text is None:
        p0_text = "%.*f" % (places, 1 - float(p1_text))
    if label is None:
        label = int(float(p1_text) > float(p0_text))
    pos = int(r.integers(0, 5000000))
    strand = "+-"[int(r.integers(0, 2))]
    return sep.join(["chr%d" % int(r.integers(1, 4)), str(pos), strand, str(5000000 - pos), "read_%d" % int(r.integers(0, 1 << 20)), "t",
                     p0_text, p1_text, str(label), KMER])


def scored_rows(seed, n, centre, places=2, spread=0.22):
    """n rows whose prob_1 lies around `centre`, rounded to `places` decimals: at two places many scores tie."""
    r = np.random.default_rng(seed)
    p1 = np.clip(r.normal(centre, spread, n), 0.0, 1.0)
    return [call_row(r, "%.*f" % (places, v)) for v in p1]


def subsample_texts(seed):
    """The two files of the subsampled golden, more than 100,000 rows each: only the seed is committed."""
    return ("\n".join(scored_rows(seed, 100400, 0.33, places=4)) + "\n", "\n".join(scored_rows(seed + 1, 100250, 0.68, places=4)) + "\n")


def load_gold():
    with open(os.path.join(HERE, "golden", "evaluate_golden.json")) as f:
        return json.load(f)


def case_texts(case):
    if "rows_seed" in case:
        return subsample_texts(case["rows_seed"])
    return case["unmethylated"], case["methylated"]


def write_inputs(tmp_path, unmethylated, methylated):
    paths = []
    for name, text in (("unmethylated.tsv", unmethylated), ("methylated.tsv", methylated)):
        p = tmp_path / name
        p.write_bytes(text if isinstance(text, bytes) else text.encode())
        paths.append(str(p))
    return paths


def run_route(tmp_path, capsys, paths, on, seed=None, num_sites=ev.NUM_SITES, **kw):
    """One route on the two files -> (result file bytes, stdout). on: "cpu", or "gpu" with the keywords of evaluate_gpu."""
    import random
    out = str(tmp_path / ("result_%s.tsv" % on))
    rng = random if seed is None else random.Random(seed)
    capsys.readouterr()
    if on == "cpu":
        ev.evaluate_cpu(paths[0], paths[1], out, num_sites, rng)
    else:
        ev.evaluate_gpu(paths[0], paths[1], out, num_sites, rng, **kw)
    with open(out, "rb") as f:
        return f.read(), capsys.readouterr().out


class CheckerBackend(RememberedBatches):
    """eval_begin .. eval_end of Engine on top of ds_eval_reference: the batches are remembered and the checker makes its one pass
    over all of them when the result is asked for."""

    def eval_begin(self, total_rows, batch_rows, cf):
        self.begun(total_rows, batch_rows)
        self.cf = np.array(cf, np.float64)

    def eval_parse(self, text, begin, end, flags):
        chunk, b, e = self.remember(text, begin, end, flags=np.array(flags, np.uint8))
        return eng.eval_reference(chunk, b, e, flags, np.zeros(len(b), np.uint8), self.cf)["status"]

    def eval_accumulate(self, mask, rows=(), p0=(), p1=(), label=()):
        assert len(mask) == len(self.batches[-1]["begin"])
        self.give({int(r): (a, b, c) for r, a, b, c in zip(rows, p0, p1, label)}, mask=np.array(mask, np.uint8))

    def eval_result(self):
        text, begin, end, (flags, mask), given, row = self.joined("flags", "mask")
        out = eng.eval_reference(text, begin, end, flags, mask, self.cf, given)
        assert not (out["status"] == eng.TEXT_ROW_HOST).any(), "a host row got no values"
        return {"counts": out["counts"], "u2": out["u2"], "p": out["p"], "n": out["n"], "rows": row}

    eval_times, eval_end = RememberedBatches.times, RememberedBatches.close
