"""Record shards: one file = a small header + one contiguous array per field (structure of arrays).

Layout of a ``*.dtgrec`` file (little endian)::

    0   8 bytes   magic  b"DTGREC\\x00\\x01"
    8   u32       version (1)
    12  u32       header length L (bytes of the JSON text that follows)
    16  L bytes   JSON: {"count": n, "fields": [{"name", "dtype", "shape", "offset"}, ...]}
    ..            each field's array [n, *shape], C order, at its 64-byte aligned ``offset``

The field list is generic on purpose (an image set has ``image`` uint8 [H, W, 3] and ``label`` int64 []; a token
shard needs no new format).  ``ShardSet`` memory-maps every shard of a directory; on open it compares each file's
size with what its header promises, so a bad file is refused before anything could be read past its end.
"""
import glob
import json
import mmap
import os
import struct

import numpy as np

MAGIC = b"DTGREC\x00\x01"
VERSION = 1
ALIGN = 64
SUFFIX = ".dtgrec"
_DTYPES = ("uint8", "int8", "int16", "uint16", "int32", "int64", "float16", "float32", "float64")


def _align(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def _layout(count, specs):
    """specs [(name, dtype, shape)] -> (JSON header bytes with the offsets filled in, total file size)."""
    def render(offsets):
        return json.dumps({"count": count, "fields": [
            {"name": n, "dtype": d, "shape": list(s), "offset": o} for (n, d, s), o in zip(specs, offsets)]},
            separators=(",", ":")).encode()
    offsets = [0] * len(specs)
    for _ in range(4):  # the offsets' digits change the header's length: iterate to the fixed point
        head = render(offsets)
        pos = _align(16 + len(head) + 24)  # room for the digits to grow
        new, end = [], pos
        for _, d, s in specs:
            new.append(_align(end))
            end = new[-1] + count * int(np.prod(s, dtype=np.int64)) * np.dtype(d).itemsize
        if new == offsets:
            return head, end  # the file ends with its last field: no tail padding
        offsets = new
    raise RuntimeError("shard layout did not converge")


def write_shard(path, **arrays):
    """Write one shard; every array's first dimension is the record count.  Field order = keyword order."""
    if not arrays:
        raise ValueError("write_shard: no fields")
    arrs = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    counts = {a.shape[0] if a.ndim else -1 for a in arrs.values()}
    if len(counts) != 1 or -1 in counts:
        raise ValueError("write_shard: fields must share their first dimension (the record count)")
    count = counts.pop()
    specs = []
    for k, a in arrs.items():
        if a.dtype.name not in _DTYPES:
            raise ValueError("write_shard: unsupported dtype %s for field %r" % (a.dtype, k))
        specs.append((k, a.dtype.name, tuple(int(d) for d in a.shape[1:])))
    head, size = _layout(count, specs)
    offsets = [f["offset"] for f in json.loads(head)["fields"]]
    tmp = path + ".part"
    with open(tmp, "wb") as f:
        f.write(MAGIC + struct.pack("<II", VERSION, len(head)) + head)
        for a, off in zip(arrs.values(), offsets):
            f.write(b"\0" * (off - f.tell()))
            f.write(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes())
        assert f.tell() == size
    os.replace(tmp, path)
    return path


class _Shard:
    def __init__(self, path):
        self.path = path
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            pre = f.read(16)
            if len(pre) < 16 or pre[:8] != MAGIC:
                raise ValueError("%s: not a dtg record shard (bad magic)" % path)
            version, hlen = struct.unpack("<II", pre[8:16])
            if version != VERSION:
                raise ValueError("%s: unsupported shard version %d" % (path, version))
            if 16 + hlen > size:
                raise ValueError("%s: truncated (header of %d bytes, file of %d)" % (path, hlen, size))
            try:
                head = json.loads(f.read(hlen).decode())
                self.count = int(head["count"])
                fields = [(str(x["name"]), str(x["dtype"]), tuple(int(d) for d in x["shape"]), int(x["offset"]))
                          for x in head["fields"]]
            except (ValueError, KeyError, TypeError) as e:
                raise ValueError("%s: unreadable shard header (%s)" % (path, e)) from e
            if self.count < 0 or not fields:
                raise ValueError("%s: bad record count or empty field list" % path)
            self.specs = tuple((n, d, s) for n, d, s, _ in fields)
            end = 16 + hlen
            for n, d, s, off in fields:
                if d not in _DTYPES or any(x < 0 for x in s):
                    raise ValueError("%s: bad spec for field %r" % (path, n))
                nbytes = self.count * int(np.prod(s, dtype=np.int64)) * np.dtype(d).itemsize
                if off % ALIGN or off < end:
                    raise ValueError("%s: field %r is misplaced (offset %d)" % (path, n, off))
                end = off + nbytes
                if end > size:
                    raise ValueError("%s: truncated (field %r ends at byte %d, file has %d)" % (path, n, end, size))
            if end != size:
                raise ValueError("%s: %d bytes after the last field" % (path, size - end))
            self._map = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if size else None
        self.arrays = {}
        for n, d, s, off in fields:
            self.arrays[n] = np.ndarray((self.count,) + s, dtype=np.dtype(d).newbyteorder("<"), buffer=self._map,
                                        offset=off)


class ShardSet:
    """Every ``*.dtgrec`` of ``directory`` in name order, memory-mapped, as one indexable record set."""

    def __init__(self, directory):
        paths = sorted(glob.glob(os.path.join(directory, "*" + SUFFIX)))
        if not paths:
            raise ValueError("no *%s shards in %s" % (SUFFIX, directory))
        self.shards = [_Shard(p) for p in paths]
        self.specs = self.shards[0].specs
        for s in self.shards[1:]:
            if s.specs != self.specs:
                raise ValueError("%s: field specs %r differ from %s's %r" % (s.path, s.specs, paths[0], self.specs))
        self.starts = np.cumsum([0] + [s.count for s in self.shards]).astype(np.int64)  # [n_shards + 1]
        self._n = int(self.starts[-1])

    def __len__(self):
        return self._n

    @property
    def fields(self):
        return {n: (d, s) for n, d, s in self.specs}

    def locate(self, indices):
        """Global indices -> (shard numbers, local indices); raises IndexError outside [0, len)."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self._n):
            raise IndexError("record index outside [0, %d)" % self._n)
        shard = np.searchsorted(self.starts, idx, side="right") - 1
        return shard, idx - self.starts[shard]

    def row_bytes(self, field):
        d, s = self.fields[field]
        return int(np.prod(s, dtype=np.int64)) * np.dtype(d).itemsize

    def addresses(self, field, indices):
        """Host addresses of the given records' rows of ``field`` (for ``dtg._runtime.gather_rows``)."""
        shard, local = self.locate(indices)
        base = np.array([s.arrays[field].ctypes.data for s in self.shards], dtype=np.int64)
        return base[shard] + local * self.row_bytes(field)

    def take(self, field, indices):
        """numpy gather of ``field`` (the slow, obviously right way; tests and small reads)."""
        shard, local = self.locate(indices)
        d, s = self.fields[field]
        out = np.empty((len(shard),) + s, dtype=d)
        for i, (sh, lo) in enumerate(zip(shard, local)):
            out[i] = self.shards[sh].arrays[field][lo]
        return out

    def close(self):
        for s in self.shards:
            s.arrays = {}
            if s._map is not None:
                try:
                    s._map.close()
                except BufferError:  # a caller still holds a view: the map goes with it
                    pass
                s._map = None
