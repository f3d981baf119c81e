"""Child process of tests/test_repair.py::test_checked_library: the repair call
against the bounds-checked build of the library (every DMA source and row store
of rs_repair compared with its share's / output's extent; one outside is skipped
and reported on stderr as "uplink_ec checked: ...").  Prints the library's build
id first, then "ok"."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from uplink_amd import _native, repair  # noqa: E402


def main():
    L = _native.load(os.path.join(ROOT, "uplink_amd", "lib", "checked", "libuplink_ec_checked.so"))
    print("build", L.ec_build_id().decode(), flush=True)
    if len(sys.argv) > 1 and sys.argv[1] == "--build-id":
        return 0
    O.build()
    k, n, ess, stripes = 29, 80, 256, 41
    plen = stripes * ess
    rng = np.random.default_rng(4151)
    seg = rng.integers(0, 256, stripes * k * ess, dtype=np.uint8)
    ref = O.FEC(k, n).encode_segment(seg, ess)
    d = torch.from_numpy(ref).cuda()
    ctx = ctypes.c_void_p()
    assert L.ec_create(k, n, ess, ctypes.byref(ctx)) == 0
    perm = [int(x) for x in rng.permutation(n)]
    nums, rest = perm[:k], perm[k:]
    for targets in (rest, rest[:3]):
        outs = repair.repair_segments(ctx, [(nums, [d[x] for x in nums], targets)])
        torch.cuda.synchronize()
        assert np.array_equal(outs[0].cpu().numpy(), ref[targets]), len(targets)
    # the share check: k + 3 shares, clean, then one byte of a surplus share flipped
    nums, targets = perm[:k + 3], perm[k + 3:k + 10]
    pieces = [d[x].clone() for x in nums]
    status = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    out = torch.empty((len(targets), plen), dtype=torch.uint8, device="cuda")
    for flip, want in ((False, 0), (True, 1)):
        if flip:  # (basis or surplus: either way some surplus share no longer agrees with the basis)
            pieces[0][plen - 1] ^= 0x40
        rc = repair.repair_call(ctx, [(nums, pieces, targets)], list(out), stripes, _native.EC_FLAG_CHECK_SHARES,
                                status)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert int(status[0]) == want, (flip, int(status[0]))
        if not flip:
            assert np.array_equal(out.cpu().numpy(), ref[targets])
    L.ec_destroy(ctx)
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
