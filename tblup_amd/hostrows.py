"""The way a generation's children take from the device to the host arrays that become their genomes.

The GPU DE step (tblup_amd.evolver) leaves the children on the device; the reference's Individual
objects need each child's genome as a numpy array.  HostRows decides how they cross and issues the
copies; the evolver only asks it for the arrays and for the moment they have landed:

* float64 children up to TBLUP_BLOCK_ROWS_MB: one DMA into a page-locked block whose rows become
  the children's genomes (views: no host copy) -- a node-shared segment when several ranks of one
  node run the generation (tblup_amd.shmrows: each rank copies its shard's rows), else a block from
  torch's caching host allocator;
* anything else: chunks, each followed by an event, so the per-row copies of one chunk into an own
  array per child overlap the transfer of the next.

_RowBlocks keeps the page-locked blocks that the population still references bounded (compaction).
"""
import os
import weakref

import numpy as np

from .keystore import TrackedGenome, track, track_rows
from .shmrows import RING as _SHM

_POOL = None


def _pool(workers=8):
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(workers, thread_name_prefix="tblup-copy")
    return _POOL


def _copy_rows(host, dtypes, workers=8, ready=None, dest=None):
    """An own array per child: float64 rows as TrackedGenome views (the key store mirrors
    them on the device and must notice in-place writes), other dtypes as plain arrays.
    ready: per-chunk callables that block until that chunk of `host` has arrived (the
    device-to-host copy is chunked so the row copies of chunk c overlap the transfer of
    chunk c + 1).  dest: preallocated float64 rows to copy into (dtypes None).  (Splitting
    each chunk over all workers measured slower: 4.3 vs 3.0 ms at config 2.)"""
    n = host.shape[0]
    nchunk = workers if ready is None else len(ready)
    step = (n + nchunk - 1) // nchunk

    def chunk(c):
        lo, hi = c * step, min(n, (c + 1) * step)
        if ready is not None:
            ready[c]()
        if dtypes is None and dest is not None:
            for i in range(lo, hi):
                np.copyto(dest[i], host[i])
            return [track(dest[i]) for i in range(lo, hi)]
        if dtypes is None:
            return [track(np.array(host[i])) for i in range(lo, hi)]
        return [np.array(host[i], dtype=dtypes[i]) for i in range(lo, hi)]
    if ready is None and n * host.shape[1] < (1 << 20):
        return [a for c in range(nchunk) for a in chunk(c)]
    parts = _pool(workers).map(chunk, range(nchunk))
    return [a for part in parts for a in part]


class _RowBlocks:
    """Page-locked blocks (one per generation) whose rows are children's genomes.

    A row is a view, so a block stays allocated while any genome in it lives (the reference
    gives every child its own array, individual.py:110-118; a view is one as far as any
    reader can tell: disjoint rows, float64, written through the TrackedGenome paths).  DE selection leaves survivors spread
    over older blocks: when more than `keep` older blocks are still referenced by the
    population, the least-referenced ones are compacted -- those individuals' genomes are
    replaced by equal own copies (set_internal_genome, individual.py:100-101) -- so at most
    keep + 2 generations (about 2 GiB) stay page-locked.  The copies run on worker threads
    while the next generation's GPU work and transfers are in flight, and the genomes are
    swapped to them at the next compaction (an own array each: they are never DMA'd again,
    their device rows stay in the key store).  Freed blocks go back to torch's caching host
    allocator and are reused without new page-locking."""

    def __init__(self, keep=12):
        self.keep = keep
        self._reg = {}   # id(block) -> weakref(block)
        self._reserved = set()
        self._pending = []   # (individual, its genome when the copy started, future of the copy)

    def keep_for(self, nbytes):
        """Older blocks kept page-locked for blocks of nbytes (about 2 GiB in all)."""
        return max(1, min(self.keep, (2 << 30) // max(nbytes, 1)))

    def reserve(self, shape):
        """Pre-size torch's caching host allocator for blocks of `shape`: the steady state holds
        keep_for + 2 blocks at once (the kept older ones, the current population's, the one being
        filled), so page-lock that many once, on the first generation -- otherwise every
        generation until the pool is full pins a fresh block (~10 ms per 100 MB).  Synchronously:
        page-locking from a background thread (round 4) contended with the generation's own HIP
        calls and made generations 2-12 slower (18 ms vs 12 ms at config 2) than pinning them
        one by one."""
        key = tuple(int(x) for x in shape)
        if key in self._reserved:
            return
        self._reserved.add(key)
        import torch
        n = self.keep_for(8 * int(np.prod(key))) + 2
        bufs = [torch.empty(key, dtype=torch.float64, pin_memory=True) for _ in range(n)]
        del bufs   # back to the caching allocator, page-locked

    def rows(self, block):
        self._reg[id(block)] = weakref.ref(block)
        rows = track_rows(block)
        block.flags.writeable = False   # the rows' private aliases are the only writable ones
        return rows

    def _block_of(self, g):
        b = g._blk if type(g) is TrackedGenome else None   # set by track_rows: no base walk
        if b is not None:
            r = self._reg.get(id(b))
            if r is not None and r() is b:
                return b
        b = g
        while isinstance(b, np.ndarray):
            r = self._reg.get(id(b))
            if r is not None and r() is b:
                return b
            b = b.base
        return None

    def finish(self, store=None):
        """Swap the members whose copies the last compaction started to those copies: skipped
        for a genome replaced or written (TrackedGenome marks it stale) since the copy began --
        it stays where it is and a later compaction takes it."""
        pending, self._pending = self._pending, []
        for indv, old, fut in pending:
            new = fut.result()
            if getattr(indv, "_genome", None) is not old or old._stale:
                continue
            t = track(new)
            indv.set_internal_genome(t)
            if store is not None:
                store.rebind(indv, old, t)

    def compact(self, individuals, store=None):
        """Blocks that only a few members of the population still use (<= n / 64 rows), and
        the least-used ones beyond `keep`: those members' genomes are copied into own arrays on
        worker threads (np.copyto releases the GIL; the copies overlap the next generation's
        transfers) and swapped by the next call (finish); the key store keeps their device rows.
        (Round 4 copied them here, on the caller's thread, into page-locked buffers: 2-12 ms per
        generation at pop 1024.)"""
        self.finish(store)
        self._reg = {k: r for k, r in self._reg.items() if r() is not None}
        if not self._reg:
            return
        users = {}
        for indv in individuals:
            g = getattr(indv, "_genome", None)
            blk = self._block_of(g) if isinstance(g, np.ndarray) else None
            if blk is not None:
                users.setdefault(id(blk), []).append(indv)
        order = sorted(users, key=lambda k: len(users[k]))
        few = max(1, len(individuals) // 64)
        # at most `keep` older blocks, fewer when they are large (about 2 GiB page-locked)
        big = max(r().nbytes for r in self._reg.values())
        keep = self.keep_for(big) - 1   # the blocks dropped here are released at the next call (finish)
        drop = [k for i, k in enumerate(order) if len(users[k]) <= few or i < len(order) - keep]
        if not drop:
            return
        moved = [indv for k in drop for indv in users[k]
                 if indv.get_internal_genome() is indv._genome]   # RandomKey / Index semantics only
        pool = _pool()
        # runs of rows per job: few pool round trips, each copy large enough to release the GIL
        per = max(1, (len(moved) + 7) // 8)
        for j0 in range(0, len(moved), per):
            grp = moved[j0:j0 + per]
            fut = pool.submit(_copy_genomes, [indv._genome for indv in grp])
            for j, indv in enumerate(grp):
                self._pending.append((indv, indv._genome, _Part(fut, j)))


def _copy_genomes(genomes):
    return [np.array(g.view(np.ndarray)) for g in genomes]


class _Part:
    """Item j of a future's list result."""

    def __init__(self, fut, j):
        self.fut, self.j = fut, j

    def result(self):
        return self.fut.result()[self.j]


_BLOCKS = _RowBlocks()

# a generation's float64 children up to this many bytes cross as one page-locked block
_BLOCK_MAX = int(os.environ.get("TBLUP_BLOCK_ROWS_MB", "1024")) << 20

# children of a generation up to this many bytes get page-locked genome buffers
_PINNED_ROWS_MAX = int(os.environ.get("TBLUP_PINNED_ROWS_MB", "2048")) << 20


def _copy_range(host, children, lo, hi):
    """children[lo:hi] -> host[lo:hi] on the current stream; the event recorded behind the copy."""
    import torch
    if lo < hi:
        host[lo:hi].copy_(children[lo:hi], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return ev


class HostRows:
    """The host arrays of one generation's `children` (n x L on the device; dtypes: the children's
    numpy dtypes, None when all float64; shard: this rank's (lo, hi) of the n children).  The copies
    are issued on the current stream when the object is made.

    whole: the block (or node-shared segment) whose rows become the genomes, None when every
    child gets an own array.  A child may be bound to a row of `whole` before landed()."""

    def __init__(self, children, dtypes, n, L, shard):
        import torch
        self._dtypes, self._n, self._L = dtypes, n, L
        block_rows = dtypes is None and n * L * 8 <= _BLOCK_MAX
        # several ranks of one node: a node-shared block, each rank copying its shard's rows
        self._shared = _SHM.acquire(children.shape, _BLOCKS.keep_for(n * L * 8)) if block_rows else None
        if self._shared is not None:
            self.whole = self._shared
            self._events = [_copy_range(torch.from_numpy(self._shared), children, *shard)]
            return
        if block_rows:
            _BLOCKS.reserve(children.shape)
        host = torch.empty(children.shape, dtype=torch.float64, pin_memory=True)
        nchunk = 1 if block_rows else (8 if n >= 16 else 1)
        rows = (n + nchunk - 1) // nchunk
        self._events = [_copy_range(host, children, c * rows, min(n, (c + 1) * rows)) for c in range(nchunk)]
        self._host = host.numpy()
        self.whole = self._host if block_rows else None

    def landed(self):
        """Wait until the rows of `whole` have arrived: the whole block (one event), every rank's shard
        of a shared one.  Own arrays per child wait chunk by chunk inside arrays() instead."""
        if self.whole is None:
            return
        self._events[-1].synchronize()
        if self._shared is not None:
            import torch.distributed as dist
            dist.barrier()

    def arrays(self):
        """One array per child: the tracked rows of `whole`, else own arrays (_copy_rows)."""
        if self.whole is not None:
            return _BLOCKS.rows(self.whole)
        # an own array per child; float64 rows go into page-locked buffers from torch's caching
        # host allocator, which hands back the buffers of dead genomes: no page faults on the copy
        dest = None
        if self._dtypes is None and self._n * self._L * 8 <= _PINNED_ROWS_MAX:
            import torch
            dest = [torch.empty(self._L, dtype=torch.float64, pin_memory=True).numpy() for _ in range(self._n)]
        return _copy_rows(self._host, self._dtypes, ready=[ev.synchronize for ev in self._events], dest=dest)
