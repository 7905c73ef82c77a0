"""The placement experiments' allocator (profiles/r03 section on staggered starts, profiles/r04/README.md sections 8 and 12): a DeviceAssembler
whose arrays are placed on purpose.  The product allocates with torch.empty alone -- the experiments are closed (placement is "a
device state") -- and tools/placement_study.py and tools/lib_ab.py use this subclass where they vary the placement.

  stagger=<bytes>     the k-th array of the assembler starts k*stagger bytes (mod 2 MiB, in steps of 256) into its allocation
  align=<bytes>       every array's size is rounded up to a multiple (the arrays of an arena then start on that grid)
  pad=<bytes>         a gap behind every array
  arena_gb=<GB>       one block is reserved and handed back to torch's caching allocator, so that every later array is carved out of that ONE
                      device allocation, back to back; arena_when="start": when the assembler is created, "outputs": in front of the first
                      output set (only the OUTPUT arrays share the allocation)"""
import torch

from otmb_amd.device import DeviceAssembler


class PlacedAssembler(DeviceAssembler):
    def __init__(self, device=0, *, stagger=0, align=0, pad=0, arena_gb=0.0, arena_when="start"):
        super().__init__(device)
        self.stagger, self.align, self.pad = int(stagger), int(align), int(pad)
        self.arena_gb, self.arena_when = float(arena_gb), arena_when
        self._nalloc = 0
        if arena_when == "start":
            self._arena()

    def _arena(self):
        if self.arena_gb > 0:
            block = torch.empty(int(self.arena_gb * 2 ** 30), dtype=torch.uint8, device=self.device)
            del block
            self.arena_gb = 0.0  # (once)

    def _empty(self, n, dtype):
        item = torch.empty(0, dtype=dtype).element_size()
        if self.align > 0 or self.pad > 0:
            nbytes = max(n * item, 1)
            if self.align > 0:
                nbytes = (nbytes + self.align - 1) // self.align * self.align
            raw = torch.empty(nbytes + self.pad, dtype=torch.uint8, device=self.device)
            return raw[: n * item].view(dtype)
        if self.stagger <= 0:
            return super()._empty(n, dtype)
        self._nalloc += 1
        off = (self._nalloc * self.stagger) % (1 << 21)
        off -= off % 256
        raw = torch.empty(n * item + off, dtype=torch.uint8, device=self.device)
        return raw[off:off + n * item].view(dtype)

    def new_output_set(self):
        if self.arena_when == "outputs":
            self._arena()
        return super().new_output_set()
