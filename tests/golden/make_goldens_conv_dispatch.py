"""Record the conv stack's host-side decisions of one build of the library.

Run:  SEL_LIB=/path/to/libsel.so python tests/golden/make_goldens_conv_dispatch.py
      SEL_LIB=/path/to/libsel.so python tests/golden/make_goldens_conv_dispatch.py --slots out.json

Without arguments writes ``conv_dispatch.npz``: sel_conv_fwd_kernel_id for every
case and tune setting of tests/conv_dispatch_cases.py (``k<key>_v<value>``
arrays), the case table itself (``cases``) and sel_dconv_kernel's answers for
the MPD chain (``dconv``).  The committed file was recorded from the library of
the commit before the forward decision was gathered into one function; a later change of a
dispatch heuristic regenerates it from its own build and says so.

--slots writes the values that depend on the device's occupancy query
(sel_resunit_wgrad_splits, sel_conv_wgrad_workspace) as JSON, to compare two
libraries on one machine.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "dl-speech-enhancement_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import conv_dispatch_cases as C  # noqa: E402
from sel import _lib as L  # noqa: E402


def main():
    lib = L.load()
    if len(sys.argv) > 2 and sys.argv[1] == "--slots":
        with open(sys.argv[2], "w") as f:
            json.dump(C.slot_values(lib), f)
        return
    cases = C.conv_cases()
    np.savez_compressed(os.path.join(HERE, "conv_dispatch.npz"), cases=np.array(cases, dtype=np.int64),
                        dconv=np.array(C.dconv_kernels(lib)), **C.forward_ids(lib, cases))


if __name__ == "__main__":
    main()
