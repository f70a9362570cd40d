"""The one Route of the side libraries' tests: the libraries a module names, all of one kind, and the memory their views, lists,
scratch and destinations live in.  [sim]: tests/sim_<name>/libbrc_<name>_sim.so (built on demand), host memory, numpy; [hip]: the
product's libraries, device memory through torch.  The libraries are rows of tests/abi_side.py's table.  Not a test module."""
import os

import numpy as np

from bam_readcount_amd import capi
import abi_side as side

SENT8, SENT = 0xA5, 0xA5A5A5A5


class Route:
    """Route(name, libs, engine): name is "sim" or "hip"; every library of `libs` becomes an attribute of its table name holding a
    handle; engine=True adds engine_lib and knob_lib (the engine's library and the one the test knobs reach), engine=False neither
    builds nor loads an engine."""

    def __init__(self, name, libs=(), engine=False):
        self.name = name
        hip = name == "hip"
        if hip:
            import torch
            self.torch = torch
        self.mem = capi.MEM_DEVICE if hip else capi.MEM_HOST
        if engine and hip:
            self.engine_lib = capi.load_product()
            # conftest's knob_lib [hip]: the product's own objects linked with the test knobs switched on
            self.knob_lib = capi.Library(os.path.join(side.CSRC, "libbrc_hip_testknobs.so"))
        elif engine:
            self.engine_lib = self.knob_lib = capi.Library(side.sim_engine())          # (the simulator reads the knobs itself)
        for lib in libs:
            setattr(self, lib, self.another(lib))

    def another(self, lib):
        """a further handle of the library `lib`, of this route's kind"""
        row = side.SIDE[lib]
        h = getattr(capi, row["cls"])(None if self.name == "hip" else side.sim_lib(row))
        assert h.kind() == ("hip-gfx950" if self.name == "hip" else "sim")
        return h

    # ---- into the route's memory: a buffer is a numpy array [sim] or a torch device tensor [hip]

    def _up(self, a):
        return self.torch.from_numpy(a).cuda() if self.name == "hip" else a

    def put(self, a):
        """the array itself where the host's memory is the route's ([sim]: no copy, dtype and shape kept, so a test may write through
        it); [hip]: a device tensor of its bytes.  Never empty."""
        a = np.ascontiguousarray(a)
        if self.name != "hip":
            return a
        b = a.view(np.uint8).reshape(-1)
        return self._up(b if b.size else np.zeros(4, np.uint8))

    def copy_bytes(self, a):
        """a fresh copy of the array's bytes (uint8, flat) on either route (never empty: an empty array still has an address)"""
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        return self._up((a if a.size else np.zeros(4, np.uint8)).copy())

    def ints(self, a):
        """an int32 list (never empty: an empty list still has an address)"""
        a = np.ascontiguousarray(a, np.int32)
        return self._up(a if a.size else np.zeros(1, np.int32))

    def sentinel_words(self, n_words):
        """n_words (at least one) 32-bit words holding SENT"""
        a = np.full(max(n_words, 1), SENT, np.uint32)
        return self._up(a.view(np.int32)) if self.name == "hip" else a

    def sentinel_bytes(self, n_bytes):
        """n_bytes (at least four) bytes of SENT8"""
        return self._up(np.full(max(n_bytes, 4), SENT8, np.uint8))

    def ptr(self, buf):
        return buf.data_ptr() if self.name == "hip" else buf.ctypes.data

    # ---- back on the host ([hip]: a copy on the default stream, behind the launches queued there)

    def host(self, buf):
        """the buffer as a numpy array of its own element type"""
        return buf.cpu().numpy() if self.name == "hip" else buf

    def words(self, buf):
        return self.host(buf).view(np.uint32)

    def quads(self, buf):
        return self.host(buf).view(np.uint64)
