"""The remembered-batches half of the CPU stand-ins for Engine's table runs (freq_cases.ReferenceBackend and the CheckerBackends of
combine_cases and evaluate_cases): a parsed batch's bytes, its spans rebased to them, its per-row columns and the values the caller
gave for its host rows are kept, and joined() makes of all batches the one input the checker takes for its one pass in row order."""
import numpy as np


class RememberedBatches:
    def __init__(self):
        self.total = self.batch = 0
        self.batches = []

    def begun(self, total_rows, batch_rows):
        self.total, self.batch, self.batches = total_rows, batch_rows, []

    def remember(self, text, begin, end, **columns):
        """A batch of a *_parse -> (its chunk of the text, begin, end inside the chunk)."""
        assert 1 <= len(begin) <= self.batch
        lo, hi = int(begin[0]), int(end[-1])
        chunk = np.asarray(text[lo:hi]).tobytes()
        b, e = np.asarray(begin, np.int64) - lo, np.asarray(end, np.int64) - lo
        self.batches.append(dict(columns, chunk=chunk, begin=b, end=e, given={}))
        return chunk, b, e

    def give(self, given: dict, **columns):
        """A *_accumulate: {batch row: the caller's values} and what else came with it, for the batch remembered last."""
        self.batches[-1].update(columns, given=given)

    def joined(self, *columns):
        """(text, begin, end, the named columns, given keyed by global row, rows) over all batches."""
        text, begin, end, given, off, row = [], [], [], {}, 0, 0
        for bt in self.batches:
            text.append(bt["chunk"]); begin.append(bt["begin"] + off); end.append(bt["end"] + off)
            given.update({row + r: v for r, v in bt["given"].items()})
            off += len(bt["chunk"]); row += len(bt["begin"])
        cols = [np.concatenate([bt[c] for bt in self.batches]) for c in columns]
        return b"".join(text), np.concatenate(begin), np.concatenate(end), cols, given, row

    def times(self, reset=False):
        return {}

    def close(self):
        pass
