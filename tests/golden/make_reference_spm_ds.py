"""Record what the reference's battery primer model (book/src/primer/src/spm.ds) evaluates to through this repository's DiffSL front end, into
tests/golden/reference_spm_ds.json: the model's dimensions and default inputs, and its right-hand side, J v and stop conditions at four seeded points and its
initial state.  tests/test_diffsl_front.py checks the built-in single-particle model (written from the same file) and the repository's own DiffSL text of it
against these numbers.  Data only: the file's text is read here and never stored.

Needs the reference checkout and a built tree (python -c "import __graft_entry__ as g; g.build()"):

    python tests/golden/make_reference_spm_ds.py <reference checkout>/book/src/primer/src/spm.ds
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_spm_ds.json")
SEED, POINTS = 4, 4


def main(path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import diffsl_models as D
    from diffsol_amd import diffsl as fe
    from oracle import oracle as O
    O.build()
    code = open(path).read()
    _, dims, defaults = fe.generate(code, fe.TARGET_HOST_C)
    mid = D.host_model(O, code)
    rng = np.random.default_rng(SEED)
    points = []
    for _ in range(POINTS):
        x = np.concatenate([rng.uniform(0, 1, 2), rng.uniform(0.2, 0.9, 20), rng.uniform(0.3, 0.95, 20)])
        p, v = rng.uniform(0.6, 1.4, 1), rng.standard_normal(42)
        points.append({"x": x.tolist(), "p": p.tolist(), "v": v.tolist(), "rhs": O.model_rhs(mid, x, p).tolist(),
                       "jac_mul": O.model_jac_mul(mid, x, p, v).tolist(), "root": O.model_root(mid, x, p).tolist()})
    rec = {"source": "reference book/src/primer/src/spm.ds through diffsol_amd.diffsl (host C target), tests/golden/make_reference_spm_ds.py",
           "dims": {k: (list(dims[k]) if k == "band" else dims[k]) for k in ("n", "nparams", "nroots", "nout", "has_mass", "band")},
           "defaults": np.asarray(defaults).tolist(), "init_inputs": [1.0], "init": O.model_init(mid, [1.0]).tolist(), "points": points}
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
