"""Records tests/golden/device_draws.npz on a GPU: the words tgp_draw_words writes, two of tgp_draw_fill's buffers and one
tgp_draw_selection, for tests/test_device_draws_cpu.py::test_numpy_generator_equals_the_device_words (the host's NumPy restatement
of the generator must reproduce them bit for bit).

    python tests/golden/make_device_draws_golden.py [output path]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(path):
    from tgpose_amd import ops
    dev = "cuda:0"
    k64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64)).to(dev)
    out = {}
    cases = [(0, 0, [0, 1, 2], 64), (2 ** 64 - 1, 0, [2 ** 64 - 1, 2 ** 63, 12345678901234567], 64), (20240229, 3, [7, 2 ** 32, 2 ** 32 + 7], 32),
             (0x0123456789abcdef, 7, np.arange(16) * 1000003, 16), (99, 0xffffffff, [5], 256)]
    for j, (seed, site, keys, n) in enumerate(cases):
        keys = np.asarray(keys, dtype=np.uint64)
        w = ops.draw_words(k64(keys), seed, site, n).cpu().numpy().view(np.uint32)
        out.update({"seed.%d" % j: np.uint64(seed), "site.%d" % j: np.uint32(site), "keys.%d" % j: keys, "words.%d" % j: w})
    out["n_cases"] = np.int32(len(cases))
    seed, keys = 424242, np.asarray([3, 2 ** 40 + 1], dtype=np.uint64)
    fill = ops.draw_fill(k64(keys), seed, 512, defor=True, drop_u=True)
    out.update({"fill.seed": np.uint64(seed), "fill.keys": keys, "fill.defor": fill["defor"].cpu().numpy(), "fill.drop_u": fill["drop_u"].cpu().numpy()})
    out.update({"sel.total": np.int32(5000), "sel.sel": ops.draw_selection(5000, k64(keys), seed, 2, 2048).cpu().numpy()})
    np.savez_compressed(path, **out)
    print("wrote", path, {k: getattr(v, "shape", ()) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "device_draws.npz"))
