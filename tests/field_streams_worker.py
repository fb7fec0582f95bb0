"""Child process of tests/test_field_streams.py: it loads build/field_streams.so and serves the harness's entry points over
its pipes, so that the HIP runtime the harness links never enters the pytest process (where torch brings its own: two HIP
runtimes in one process leave the later one without a device).

Protocol, both ways: an 8-byte little-endian length, then a pickle.  Request: (entry point, arguments), arguments being ints
and numpy arrays.  Reply: (return code, the arrays as the call left them).  The worker ends when its input closes."""
import ctypes
import os
import pickle
import struct
import sys

import numpy as np

ENTRY_POINTS = ("streams_product", "streams_predicated", "streams_chain", "streams_linear")


def main():
    out = os.fdopen(os.dup(1), "wb", buffering=0)
    os.dup2(2, 1)                            # whatever a library prints goes to stderr, not into the protocol
    inp = sys.stdin.buffer
    lib = ctypes.CDLL(sys.argv[1])
    while True:
        head = inp.read(8)
        if len(head) < 8:
            return 0
        name, args = pickle.loads(inp.read(struct.unpack("<Q", head)[0]))
        if name not in ENTRY_POINTS:
            return 2
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        arrays = [np.ascontiguousarray(a) for a in args if isinstance(a, np.ndarray)]
        it = iter(arrays)
        rc = fn(*[next(it).ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else ctypes.c_int(a) for a in args])
        payload = pickle.dumps((rc, arrays))
        out.write(struct.pack("<Q", len(payload)) + payload)


if __name__ == "__main__":
    sys.exit(main())
