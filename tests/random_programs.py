"""Seeded random postfix programs (a helper module, imported by tests/test_planner.py and tools/plan_hash.py): well-formed random trees over a
few head terms — AND / OR / NOT / Optional / matchsome at any depth: CNFs, truth-table trees and TASK_TREE trees among them — and raw token
noise (operands missing, counts of zero, term ids past the dictionary, thresholds above the operand count, words that are no operator)."""
import numpy as np

import trinity_amd as T


def random_program(rng, wellformed):
    """One program drawn from `rng` (a numpy Generator; the draws of a call depend on `wellformed` and on the generator's state alone)."""
    if wellformed:  # a random postfix tree over a few terms
        st, out = 0, []
        for _ in range(int(rng.integers(1, 14))):
            if st >= 2 and rng.random() < 0.45:
                op = int(rng.choice([T.OP_AND, T.OP_OR, T.OP_NOT, T.OP_OPT, T.OP_SOME]))
                n = 2 if op in (T.OP_NOT, T.OP_OPT) else int(rng.integers(2, st + 1))
                out.append(T.tok(op, n | ((int(rng.integers(1, n + 1)) << 16) if op == T.OP_SOME else 0)))
                st -= n - 1
            else:
                out.append(T.tok(T.OP_TERM, int(rng.integers(0, 40))))
                st += 1
        if st > 1:
            out.append(T.tok(T.OP_AND, st))
        return np.array(out, dtype=np.uint32)
    n = int(rng.integers(1, 12))
    ops = rng.integers(0, 8, size=n)  # (7: not an operator at all)
    args = np.where(rng.random(n) < 0.7, rng.integers(0, 6, size=n), rng.integers(0, 1 << 28, size=n))
    return ((ops.astype(np.uint32) << 28) | args.astype(np.uint32)).astype(np.uint32)
