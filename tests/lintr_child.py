"""Child process of tests/test_gpu_lintr.py: draws the small mixed LINTR layout under the three
plans in a fresh process (so that TWOSD_LINTR_CHUNK, read at call time, is whatever the parent put
into the environment) and writes the streams to the .npz named on the command line."""
import sys

import numpy as np


def main(out):
    from tests import test_gpu_lintr as T
    ctx, _ = T.small("exact")
    got = {T.plan_name(plan): T.draw(ctx, T.N_SMALL, T.SEED, T.FIRST, plan) for plan in T.PLANS}
    np.savez(out, **got)
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1])
