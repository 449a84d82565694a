#!/usr/bin/env python3
"""Records ragged_tables_host.json: what the four host plans of the ragged-batch layers - ops.EvalTables, ops.SeqTable,
ops.ShotTables and ops.FusionTables - build, or refuse, over a corpus of offsets and pair lists.  Everything is built
with device="cpu": no GPU and no library call.  tests/test_ragged_host.py replays the file against the tree under test,
so record it from a checkout of the commit BEFORE a change to the plans (pass that checkout's root), never from the tree
being changed:

    python tests/golden/make_ragged_tables_golden.py path/to/parent/checkout

An accepted case stores every public attribute, device-side tensors included, as lists; an array of more than 64
entries is stored as shape, dtype and the SHA-256 of its little-endian bytes.  A refused case stores the exception's
type name.  Equal array records (a table's offsets, their device copy, the same offsets under another class) are kept once,
in "arrays", and referred to by position; expand() puts them back."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
INLINE = 64
LAYOUT = [7, 9, 265, 522, 2322, 2325]


def offset_inputs():
    """[label, form, values]: ``form`` says how build_offsets hands the values over."""
    fixed = [[], [0], [0, 1], [0, 2], [0, 5, 5], [0, 5, 3], [1, 4], [-2, 5], LAYOUT,
             [0, 32768], [0, 32769], [0, 2, 32770],                                     # the EvalTables length limits
             [0, 1 << 24], [0, (1 << 24) + 1],                                          # the ShotTables total limits
             [0, (1 << 31) - 1], [0, 1 << 31], [(1 << 31) - 10, (1 << 31) + 10]]        # the 2^31 limits
    out = [[str(v), "list", v] for v in fixed]
    one = [0, 3, 260, 2308, 2310]
    out += [[f"{form} {one}", form, one] for form in ("np_int32", "torch_int64", "nested", "floats")]
    rng = np.random.default_rng(20251)
    for i in range(50):
        lengths = rng.integers(1, 3001, int(rng.integers(1, 41)))
        out.append([f"random {i}", "list", [0] + np.cumsum(lengths).tolist()])
    return out


def build_offsets(form, values):
    if form == "np_int32":
        return np.asarray(values, dtype=np.int32)
    if form == "torch_int64":
        return torch.tensor(values, dtype=torch.int64)
    if form == "nested":
        return [[v] for v in values]
    if form == "floats":
        return [float(v) for v in values]
    return list(values)


def pair_inputs():
    """[label, pairs]: lists of (v_row0, n, a_row0, m)."""
    def packed(shapes, gap=0):
        pairs, rv, ra = [], 0, 0
        for n, m in shapes:
            pairs.append([rv + gap, n, ra + 2 * gap, m])
            rv, ra = rv + gap + n, ra + 2 * gap + m
        return pairs
    edges = (1, 64, 65, 512, 513)
    classes = [(l, l) for l in edges] + [(l, 700) for l in edges] + [(700, l) for l in edges]
    out = [["empty list", []], ["class boundaries", packed(classes)], ["class boundaries with gaps", packed(classes, 5)],
           ["class boundaries shuffled", [packed(classes, 3)[i] for i in np.random.default_rng(5).permutation(len(classes))]],
           ["n = 6400", packed([(3, 3), (6400, 5)])], ["n = 6401", packed([(3, 3), (6401, 5)])],
           ["n = 0", [[0, 3, 0, 3], [3, 0, 3, 4]]], ["m = 0", [[0, 3, 0, 3], [3, 4, 3, 0]]],
           ["negative v_row0", [[-1, 3, 0, 3]]], ["negative a_row0", [[0, 3, -4, 3]]]]
    rng = np.random.default_rng(20252)
    for i in range(20):
        count = int(rng.integers(1, 201))
        shapes = [(int(rng.integers(1, 701)), int(rng.integers(1, 701))) for _ in range(count)]
        pairs = packed(shapes, int(rng.integers(0, 4)))
        out.append([f"random {i}", [pairs[j] for j in rng.permutation(count)] if i % 2 else pairs])
    return out


def cases(corpus):
    """(id, class name, constructor arguments) of every case of the corpus, in the order of the recording."""
    for label, form, values in corpus["offsets"]:
        yield f"EvalTables | {label}", "EvalTables", (build_offsets(form, values), "cpu")
        last = values[-1] if values else 0
        for rows, tag in ((None, "None"), (last, "last"), (last + 1, "last + 1")):
            yield f"SeqTable rows={tag} | {label}", "SeqTable", (build_offsets(form, values), rows, "cpu")
        for msl in (0, 1, 15):
            yield f"ShotTables min_scene_len={msl} | {label}", "ShotTables", (build_offsets(form, values), msl, "cpu")
    for label, pairs in corpus["pairs"]:
        yield f"FusionTables | {label}", "FusionTables", ([tuple(p) for p in pairs], "cpu")


def encode(x):
    if isinstance(x, torch.device):
        return str(x)
    if isinstance(x, torch.Tensor):
        return {"torch": str(x.dtype), "value": encode(x.numpy())}
    if isinstance(x, np.ndarray):
        rec = {"dtype": str(x.dtype), "shape": list(x.shape)}
        if x.size > INLINE:
            rec["sha256"] = hashlib.sha256(np.ascontiguousarray(x).astype(x.dtype.newbyteorder("<")).tobytes()).hexdigest()
        else:
            rec["data"] = x.reshape(-1).tolist()
        return rec
    if isinstance(x, (list, tuple)):
        return [encode(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    raise TypeError(f"attribute of type {type(x).__name__}")


def attributes(obj, names=None):
    """The public attributes of a plan, encoded; ``names``: these only (what a recording holds)."""
    names = sorted(k for k in vars(obj) if not k.startswith("_")) if names is None else names
    return {k: encode(getattr(obj, k)) for k in names}


def replay(ops, corpus, recorded=None):
    """{id: {"ok": attributes} | {"error": type name, "message": text}} of ``ops``' plans over the corpus.  With
    ``recorded`` (an earlier replay), an accepted case lists the attributes that recording holds."""
    out = {}
    for key, cls, args in cases(corpus):
        try:
            obj = getattr(ops, cls)(*args)
        except Exception as e:                                  # noqa: BLE001 - the type is what is recorded
            out[key] = {"error": type(e).__name__, "message": str(e)}
            continue
        names = sorted(recorded[key]["ok"]) if recorded is not None and "ok" in recorded[key] else None
        out[key] = {"ok": attributes(obj, names)}
    return out


def _walk(x, leaf):
    if isinstance(x, dict) and "dtype" in x:
        return leaf(x)
    if isinstance(x, dict):
        return {k: _walk(v, leaf) for k, v in x.items()}
    return [_walk(v, leaf) for v in x] if isinstance(x, list) else x


def intern(results):
    """(results with every array record replaced by {"array": position}, the list of distinct records)."""
    pool = {}
    out = _walk(results, lambda rec: {"array": pool.setdefault(json.dumps(rec, sort_keys=True), len(pool))})
    return out, [json.loads(k) for k in pool]


def expand(corpus):
    """The recorded results with the array records back in place: the layout replay() returns."""
    arrays = corpus["arrays"]

    def back(x):
        if isinstance(x, dict) and "array" in x:
            return arrays[x["array"]]
        if isinstance(x, dict):
            return {k: back(v) for k, v in x.items()}
        return [back(v) for v in x] if isinstance(x, list) else x
    return back(corpus["results"])


def main():
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from avsum_amd import ops
    corpus = json.loads(json.dumps({"offsets": offset_inputs(), "pairs": pair_inputs()}))
    results = replay(ops, corpus)
    for r in results.values():
        r.pop("message", None)
    corpus["results"], corpus["arrays"] = intern(results)
    with open(os.path.join(HERE, "ragged_tables_host.json"), "w") as f:
        json.dump(corpus, f, separators=(",", ":"))
        f.write("\n")
    print(len(results), "cases,", sum("error" in r for r in results.values()), "refused; recorded from", ops.__file__)


if __name__ == "__main__":
    main()
