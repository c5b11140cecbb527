"""Host bookkeeping of STEP's evaluation cache (``STEP.eval_cache_bytes``): which windows of a resident series have their
frozen branch -- the last patch's hidden state [N, 96] f32 and the kNN prior [N, N] as one bit per edge -- stored in HBM, in
which slot, and within which budget.  Slot assignment is pure host code (no device call, no synchronisation); the only device
objects are the storage chunks, created by ``alloc`` (tests pass a recorder).  The two launches that move the data are
``step_frozen_cache_store`` / ``step_frozen_cache_load`` (include/step_hip.h), issued by step.py with the slots planned here.
"""
import torch


def window_bytes(N):
    """bytes one stored window takes: [N, 96] f32 rows + [N, ceil(N / 32)] uint32 words of prior bits"""
    return int(N) * 96 * 4 + int(N) * ((int(N) + 31) // 32) * 4


def window_keys(ref, channel=0):
    """-> one key per window of a LongHistoryRef batch, or None when the batch has no host identity (a plain tensor, or a reference
    built from device origins only: reading them back would make the host wait for the device).  A key is (identity of the
    resident series tensor, its version, the data channel the TSFormer reads, forecast origin)."""
    t0 = getattr(ref, "t0_host", None)
    if t0 is None:
        return None
    d = ref.data
    head = (id(d), d._version, int(ref.channels[channel]))
    return [head + (int(t),) for t in t0]


def new_stats():
    return {"window_hits": 0, "window_misses": 0, "windows_stored": 0, "windows_refused": 0, "invalidations": 0, "g_reuses": 0}


def _device_alloc(device):
    def alloc(windows, N):
        W = (N + 31) // 32
        return (torch.empty(windows, N, 96, device=device, dtype=torch.float32),
                torch.empty(windows, N, W, device=device, dtype=torch.int32))          # (bit patterns of the uint32 words)
    return alloc


class FrozenBranchCache:
    """Slots of stored windows.  Storage grows in chunks of ``chunk_windows`` windows as windows arrive and never above
    ``budget_bytes``; nothing is evicted: once the budget is used up, further windows are refused (computed, not stored).
    ``tie`` is whatever the stored values depend on besides the window (the TSFormer's weights and operand type, the number of
    patches, k, N): the owner compares it before every use and drops the cache when it differs."""

    def __init__(self, budget_bytes, N, tie, alloc, chunk_windows=256):
        self.budget, self.N, self.tie, self.alloc = int(budget_bytes), int(N), tie, alloc
        self.chunk_windows = max(1, int(chunk_windows))
        self.per_window = window_bytes(N)
        self.slots = {}              # window key -> global slot (chunk = slot // chunk_windows, local slot = slot % chunk_windows)
        self.chunks = []             # (cache_last, cache_bits, capacity)
        self.capacity = 0            # windows the chunks hold
        self.series = {}             # id -> the series tensors of the stored windows: kept alive so that an address is not reused

    @property
    def bytes_held(self):
        return self.capacity * self.per_window

    def lookup(self, keys):
        """-> global slot (or None) per key"""
        return [self.slots.get(k) for k in keys]

    def is_hit(self, keys):
        """a batch is a hit when ALL its windows are stored"""
        return bool(keys) and all(k in self.slots for k in keys)

    def _grow(self):
        room = (self.budget - self.bytes_held) // self.per_window
        n = min(self.chunk_windows, room)
        if n <= 0:
            return False
        last, bits = self.alloc(n, self.N)
        self.chunks.append((last, bits, n))
        self.capacity += n
        return True

    def assign(self, keys, series=None):
        """Give every window that is not stored yet a slot -> (global slot or -1 per key, windows newly stored, windows refused).
        -1: already stored (nothing to write) or refused for budget."""
        out, stored, refused = [], 0, 0
        for k in keys:
            if k in self.slots:
                out.append(-1)
                continue
            if len(self.slots) >= self.capacity and not self._grow():
                out.append(-1)
                refused += 1
                continue
            s = len(self.slots)
            self.slots[k] = s
            out.append(s)
            stored += 1
            if series is not None:
                self.series[id(series)] = series
        return out, stored, refused

    def plan(self, slots):
        """global slots of a batch (None / -1: skip) -> [(chunk index, local slot per sample with -1 where the sample lives elsewhere)],
        one entry per chunk touched: one launch each -- a single one unless the batch straddles a chunk boundary"""
        by_chunk = {}
        for i, s in enumerate(slots):
            if s is None or s < 0:
                continue
            c = s // self.chunk_windows
            by_chunk.setdefault(c, [-1] * len(slots))[i] = s % self.chunk_windows
        return sorted(by_chunk.items())
