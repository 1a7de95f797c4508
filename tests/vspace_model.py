"""A sequential model of the replicated page table: VSpace::map_generic, resolve_addr and
VSpaceDispatcher of the reference's benches/vspace.rs (:177-381, :436-467, :499-526) over a list
of 512-entry tables.

This is a restatement by hand: no Rust toolchain builds the reference here, so the model is not
pinned to it by a recorded run (the standing oracle/make_golden.py's models have). PTE runs are
numpy slices, so a 65,535-page op is cheap.

Inner entries hold table_index * 4096 | P|RW|US where the reference stores heap pointers; nothing
observable (responses, resolve, the leaf dump, the table count) depends on them.
"""
import numpy as np

P, RW, US, PS, XD = 1, 2, 4, 0x80, 1 << 63
ADDR = 0x000F_FFFF_FFFF_F000
INNER = P | RW | US
KB4, MB2, GB1 = 1 << 12, 1 << 21, 1 << 30
MAP, MAP_DEVICE = 0, 1
READ_WRITE_USER = 3

# MapAction::to_pt_rights / to_pd_rights (:92-122), by MapAction order 1..8
RIGHTS = {1: XD, 2: US | XD, 3: RW | XD, 4: RW | US | XD, 5: 0, 6: US, 7: RW, 8: RW | US}


def in_domain(vbase, pbase, length, op, rights):
    if (vbase | pbase | length) & 4095:
        return False
    if vbase >= 1 << 48 or pbase >= 1 << 48 or length >= GB1 or vbase + length > 1 << 48:
        return False
    if op == MAP:
        return 1 <= rights <= 8
    return op == MAP_DEVICE


class VSpaceModel:
    def __init__(self):
        self.t = [np.zeros(512, np.uint64)]  # table 0: the PML4

    def tables(self):
        return len(self.t)

    def _new(self):
        self.t.append(np.zeros(512, np.uint64))
        return ((len(self.t) - 1) << 12) | INNER

    def _table(self, entry):
        return self.t[(int(entry) & ADDR) >> 12]

    def map_generic(self, vbase, pbase, psize, rights):
        """None for Ok, else the error's `at`. Each turn of the loop is one recursion (frame)."""
        fl = P | RIGHTS[rights]
        while True:
            pml4 = self.t[0]
            i4 = (vbase >> 39) & 511
            if not int(pml4[i4]) & P:
                pml4[i4] = self._new()
            pdpt = self._table(pml4[i4])
            i3 = (vbase >> 30) & 511
            if not int(pdpt[i3]) & P:
                assert psize < GB1  # the 1 GiB path (:217-261) is outside the domain
                pdpt[i3] = self._new()
            pd = self._table(pdpt[i3])
            i2 = (vbase >> 21) & 511
            if not int(pd[i2]) & P:
                if vbase % MB2 == 0 and pbase % MB2 == 0 and psize >= MB2:
                    mapped = 0
                    while mapped < psize and psize - mapped >= MB2 and i2 < 512:
                        if int(pd[i2]) & P:
                            return vbase
                        pd[i2] = (pbase + mapped) | fl | PS
                        i2 += 1
                        mapped += MB2
                    if mapped < psize:
                        vbase, pbase, psize = vbase + mapped, pbase + mapped, psize - mapped
                        continue
                    return None
                pd[i2] = self._new()
            if int(pd[i2]) & PS:
                return vbase
            pt = self._table(pd[i2])
            i1 = (vbase >> 12) & 511
            n = min(psize >> 12, 512 - i1)
            present = np.flatnonzero(pt[i1:i1 + n] & np.uint64(P))
            k = int(present[0]) if len(present) else n
            pt[i1:i1 + k] = (np.uint64(pbase) + np.arange(k, dtype=np.uint64) * np.uint64(KB4)) | np.uint64(fl)
            if k < n:
                return vbase
            mapped = n * KB4
            if mapped < psize:
                vbase, pbase, psize = vbase + mapped, pbase + mapped, psize - mapped
                continue
            return None

    def dispatch_mut(self, vbase, pbase, length, op, rights):
        """(some, a, b) as the C ABI answers; an out-of-domain record changes nothing."""
        if not in_domain(vbase, pbase, length, op, rights):
            return 0, vbase, 0
        at = self.map_generic(vbase, pbase, length, rights if op == MAP else READ_WRITE_USER)
        if at is not None:
            return 0, at, 0
        return (1, pbase, length) if op == MAP else (1, 0, 0)

    def replay(self, recs):
        """recs: a VSPACE_OP_DTYPE array; -> (a, b, some) arrays"""
        a = np.zeros(len(recs), np.uint64)
        b = np.zeros(len(recs), np.uint64)
        some = np.zeros(len(recs), np.uint8)
        for i, r in enumerate(recs):
            some[i], a[i], b[i] = self.dispatch_mut(int(r["vbase"]), int(r["pbase"]), int(r["len"]), int(r["op"]),
                                                    int(r["rights"]))
        return a, b, some

    def resolve(self, addr):
        """Identify: (paddr or 0, found)"""
        e = int(self.t[0][(addr >> 39) & 511])
        if not e & P:
            return 0, 0
        e = int(self._table(e)[(addr >> 30) & 511])
        if not e & P:
            return 0, 0
        e = int(self._table(e)[(addr >> 21) & 511])
        if not e & P:
            return 0, 0
        if e & PS:
            return (e & ADDR) + (addr & (MB2 - 1)), 1
        e = int(self._table(e)[(addr >> 12) & 511])
        if not e & P:
            return 0, 0
        return (e & ADDR) + (addr & 4095), 1

    def dump(self):
        """every leaf as (vaddr, entry) arrays, ascending vaddr"""
        va, en = [], []
        for i4 in np.flatnonzero(self.t[0] & np.uint64(P)):
            pdpt = self._table(self.t[0][i4])
            for i3 in np.flatnonzero(pdpt & np.uint64(P)):
                pd = self._table(pdpt[i3])
                for i2 in np.flatnonzero(pd & np.uint64(P)):
                    base = (int(i4) << 39) | (int(i3) << 30) | (int(i2) << 21)
                    if int(pd[i2]) & PS:
                        va.append(np.array([base], np.uint64))
                        en.append(pd[i2:i2 + 1].copy())
                    else:
                        pt = self._table(pd[i2])
                        i1 = np.flatnonzero(pt & np.uint64(P))
                        va.append(np.uint64(base) + i1.astype(np.uint64) * np.uint64(KB4))
                        en.append(pt[i1])
        if not va:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        return np.concatenate(va), np.concatenate(en)


def bench_ops(rng, n, dtype):
    """n write ops drawn as generate_operations draws them (:528-554): vbase and pbase any 4 KiB
    multiple below 2^48, len any 4 KiB multiple below 2^28, Map (ReadWriteUser) or MapDevice; a
    region that would cross 2^48 is drawn again."""
    r = np.zeros(n, dtype)
    for i in range(n):
        while True:
            vbase = int(rng.integers(0, 1 << 36)) << 12
            length = int(rng.integers(0, 1 << 16)) << 12
            if vbase + length <= 1 << 48:
                break
        r[i] = (vbase, int(rng.integers(0, 1 << 36)) << 12, length, int(rng.integers(0, 2)), READ_WRITE_USER)
    return r
