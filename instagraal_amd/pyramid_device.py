"""The pyramid builder with the contact levels on the device.

``build`` and ``build_and_filter`` write the same folders as their namesakes in ``pyramid.py``: every text file byte for byte the same,
every matrix of the ``SparseStore`` equal, the same ``Pyramid`` returned.  The fragment and contig tables stay the host code they are
(``pyramid.subsample_tables``, ``pyramid.filter_tables``: O(fragments), dominated by writing their text).  What changes is the contact
side: the level-0 list is read with one vectorised parse (or handed over in memory: ``level0``), uploaded once, and every further
level -- the filtered level 0, then one binning after the other -- is made from the level before it ON the device
(``hip_lib.Context.pyr_*``), which only hands back each level's three int32 rows for its contact file and its matrix.

``device=False`` runs the same chain through the rule itself (``pyramid_levels``, numpy): the same files again, no GPU.

The reuse rules are ``pyramid._bin_levels``': a level's files are reused when they exist, a matrix when ``store.done`` is set; a level
the chain does not hold is read back from its contact file.  A list that is not canonical (``pyramid_levels.canonical``: possible only
for the input's own list) gets its one matrix from the host function ``pyramid.fill_sparse_pyramid_level``, whose column order is
the order of first appearance in the file; the device only reports that the list is not canonical.
"""
from __future__ import annotations

import os
import shutil
import time

import numpy as np

from . import pyramid as pyr
from . import pyramid_levels as rule

WRITE_ROWS = 1 << 16  # contact lines formatted at a time


def read_contacts(path):
    """one vectorised parse of a contact file -> (a, b, count), int64, file order"""
    with open(path, "rb") as f:
        f.readline()
        text = f.read()
    flat = np.fromstring(text, dtype=np.int64, sep=" ") if text.strip() else np.zeros(0, np.int64)  # (any white space separates)
    if flat.size % 3:
        raise ValueError("%s: %d numbers are not three per line" % (path, flat.size))
    t = flat.reshape(-1, 3)
    return np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1]), np.ascontiguousarray(t[:, 2])


def write_contacts(path, data3):
    """a level's contact file from its three rows: ``"%d\\t%d\\t%d\\n"`` lines under the header of ``pyramid._write_table``"""
    with open(path, "w") as f:
        f.write("\t".join(pyr.CONTACT_HEADER) + "\n")
        n = data3.shape[1]
        for a in range(0, n, WRITE_ROWS):
            block = np.ascontiguousarray(data3[:, a:a + WRITE_ROWS].T)
            f.write(("%d\t%d\t%d\n" * block.shape[0]) % tuple(block.ravel().tolist()))


class _RuleEngine:
    """the chain through ``pyramid_levels`` (``device=False``)"""

    def begin(self, n_frags, a, b, count):
        self.n, self.cur, self.is_level = int(n_frags), (a, b, count), False
        return rule.canonical(a, b)

    def matrix(self, level):
        if not self.is_level:
            self.cur, self.is_level = rule.level_matrix(*self.cur, level=level), True

    def degrees(self):
        return rule.degrees(self.cur, self.n)

    def remap(self, lut, n_new, skip_first, level):
        sc = {}
        self.cur, self.is_level, self.n = rule.remap(*self.cur, lut, skip_first, level=level, scalars=sc), True, int(n_new)
        return sc

    def level(self):
        return rule.data3(self.cur)

    def end(self):
        self.cur = None


class _DeviceEngine:
    """the chain on the device: one ``pyr`` session of a context (the caller's, or one of its own)"""

    def __init__(self, device):
        from . import hip_lib

        self.hip_lib = hip_lib
        self.ctx = device if isinstance(device, hip_lib.Context) else hip_lib.Context(0 if device is True else int(device))
        self.own = self.ctx is not device
        self.live = False

    def _call(self, level, f, *args):
        try:
            return f(*args)
        except self.hip_lib.HipError as e:  # the refusal of a sum >= 2^31 names the pixel; the level is known here
            if "2^31 or more" in str(e):
                raise rule.LevelOverflow("level %s: %s" % (level, e)) from e
            raise

    def begin(self, n_frags, a, b, count):
        if a.size and (min(int(a.min()), int(b.min())) < -(1 << 31) or max(int(a.max()), int(b.max())) >= 1 << 31):
            raise ValueError("an id of the contact list is outside 32 bits")
        flag = self.ctx.pyr_begin(n_frags, a.astype(np.int32), b.astype(np.int32), count)
        self.live = True
        return flag

    def matrix(self, level):
        self._call(level, self.ctx.pyr_matrix)

    def degrees(self):
        return self.ctx.pyr_degrees()

    def remap(self, lut, n_new, skip_first, level):
        return self._call(level, self.ctx.pyr_remap, lut, n_new, skip_first)

    def level(self):
        return self.ctx.pyr_level()[0]

    def end(self):
        if self.live:
            self.ctx.pyr_end()
            self.live = False

    def close(self):
        self.end()
        if self.own:
            self.ctx.close()


class Chain:
    """The level the engine holds and which (folder, level) it is.  ``seconds``: where the time went (read, tables, device, write)."""

    def __init__(self, device):
        self.device = device
        self.engine = None
        self.key = None
        self.is_canonical = True
        self.is_level = False
        self.seconds = dict(read=0.0, tables=0.0, device=0.0, write=0.0)

    def _timed(self, what, f, *args, **kw):
        t0 = time.perf_counter()
        try:
            return f(*args, **kw)
        finally:
            self.seconds[what] += time.perf_counter() - t0

    def ensure(self, key, contact_file, n_frags, level0=None):
        """the engine holds the list of ``key``: as it does already, from ``level0`` (a, b, count) or from the contact file"""
        if self.key == key:
            return
        a, b, count = level0 if level0 is not None else self._timed("read", read_contacts, contact_file)
        a, b, count = (np.ascontiguousarray(x, np.int64).ravel() for x in (a, b, count))
        if self.engine is None:
            self.engine = _RuleEngine() if self.device is False else _DeviceEngine(self.device)
        self.engine.end()
        self.is_canonical = self._timed("device", self.engine.begin, n_frags, a, b, count)
        self.key, self.is_level = key, False

    def matrix(self):
        self._timed("device", self.engine.matrix, self.key[1])
        self.is_level = True

    def degrees(self):
        return self._timed("device", self.engine.degrees)

    def remap(self, lut, n_new, skip_first, key):
        sc = self._timed("device", self.engine.remap, lut, n_new, skip_first, key[1])
        self.key, self.is_level = key, True
        return sc

    def level(self):
        return self._timed("device", self.engine.level)

    def close(self):
        if self.engine is not None:
            (self.engine.close if hasattr(self.engine, "close") else self.engine.end)()
            self.engine = None
        self.key = None


def _levels(chain, store, pyramid_folder, size_pyramid, factor, min_bin_per_contig, level0=None, fetched=None):
    """``pyramid._bin_levels`` with the contact side through the chain.  ``fetched``: (key, data3) of the level fetched last -- its
    contact file and its matrix are the same three rows, fetched once"""
    _, cur_contigs, cur_frags, cur_contacts, cur_index = pyr._level_paths(pyramid_folder, 0)
    nfrags = pyr.file_len(cur_frags) - 1
    for level in range(size_pyramid):
        d, contigs, frags, contacts, index = pyr._level_paths(pyramid_folder, level)
        os.makedirs(d, exist_ok=True)
        key = (pyramid_folder, level)
        if level > 0:
            if all(os.path.exists(x) for x in (contigs, frags, contacts, cur_index)):
                nfrags = pyr.file_len(frags) - 1
            else:
                chain.ensure((pyramid_folder, level - 1), cur_contacts, nfrags, level0 if level == 1 else None)
                old2new, nfrags = chain._timed("tables", pyr.subsample_tables, cur_contigs, cur_frags, factor, min_bin_per_contig, contigs, frags, cur_index)
                if factor <= 1:  # the level below once more: its file is copied, the chain's level stays
                    shutil.copy(cur_contacts, contacts)
                    chain.key = key
                else:
                    chain.remap(old2new - 1, nfrags, True, key)
                    fetched = (key, chain.level())
                    chain._timed("write", write_contacts, contacts, fetched[1])
        if not store.done(level):
            chain.ensure(key, contacts, nfrags, level0 if level == 0 else None)
            if not chain.is_level and not chain.is_canonical:
                pyr.fill_sparse_pyramid_level(store, level, contacts, nfrags)  # the reference's order of first appearance: host
            else:
                if not chain.is_level:
                    chain.matrix()
                if fetched is None or fetched[0] != key:
                    fetched = (key, chain.level())
                store.put(level, fetched[1], nfrags)
        cur_contigs, cur_frags, cur_contacts, cur_index = contigs, frags, contacts, index


def _device_of(device, chain):
    return chain if chain is not None else Chain(device)


def build(base_folder, size_pyramid, factor, min_bin_per_contig, output_folder=None, device=True, level0=None, _chain=None):
    """``pyramid.build``: the unfiltered pyramid ``pyramids/pyramid_<n>_no_thresh``.  ``level0 = (a, b, count)``: the input's contact
    list in memory (0-based ids, file order), e.g. ``pre``'s pixels; the contact text is then copied but not read."""
    root = output_folder if output_folder is not None else base_folder
    folder = os.path.join(root, "pyramids", "pyramid_%d_no_thresh" % size_pyramid)
    d0, contigs0, frags0, contacts0, _ = pyr._level_paths(folder, 0)
    os.makedirs(d0, exist_ok=True)
    chain = _device_of(device, _chain)
    try:
        shutil.copyfile(os.path.join(base_folder, "info_contigs.txt"), contigs0)
        shutil.copyfile(os.path.join(base_folder, "abs_fragments_contacts_weighted.txt"), contacts0)
        chain._timed("tables", pyr.init_frag_list, os.path.join(base_folder, "fragments_list.txt"), frags0)
        store = pyr.SparseStore(folder)
        _levels(chain, store, folder, size_pyramid, factor, min_bin_per_contig, level0)
        store.close()
    finally:
        if _chain is None:
            chain.close()
    return folder


def build_and_filter(base_folder, size_pyramid, factor, thresh_factor=1, output_folder=None, device=True, level0=None, _chain=None):
    """``pyramid.build_and_filter``: ``pyramids/pyramid_1_no_thresh``, its filtered copy as level 0 of
    ``pyramids/pyramid_<n>_thresh_auto``, then the binned levels; returns the loaded ``Pyramid``.  ``device``: True (device 0), a
    device id, a ``hip_lib.Context``, or False (the rule in numpy).  ``level0`` as in ``build``."""
    root = output_folder if output_folder is not None else base_folder
    os.makedirs(os.path.join(root, "pyramids"), exist_ok=True)
    init_folder = os.path.join(root, "pyramids", "pyramid_1_no_thresh")
    chain = _device_of(device, _chain)
    try:
        if not os.path.exists(init_folder):
            build(base_folder, 1, factor, 1, output_folder=root, device=device, level0=level0, _chain=chain)
        _, contigs_i, frags_i, contacts_i, _ = pyr._level_paths(init_folder, 0)
        folder = os.path.join(root, "pyramids", "pyramid_%d_thresh_auto" % size_pyramid)
        d0, contigs0, frags0, contacts0, _ = pyr._level_paths(folder, 0)
        os.makedirs(d0, exist_ok=True)
        fetched = None
        if not all(os.path.exists(x) for x in (contigs0, frags0, contacts0)):
            nfrags_i = pyr.file_len(frags_i) - 1
            chain.ensure((init_folder, 0), contacts_i, nfrags_i, level0)
            chain.matrix()  # (of a list that is not canonical too: the degrees and the filtered level are sums)
            deg = chain.degrees()
            lut, _ = chain._timed("tables", pyr.filter_tables, contigs_i, frags_i, contigs0, frags0, deg, nfrags_i, thresh_factor=thresh_factor)
            chain.remap(lut, pyr.file_len(frags0) - 1, False, (folder, 0))
            fetched = ((folder, 0), chain.level())
            chain._timed("write", write_contacts, contacts0, fetched[1])
        store = pyr.SparseStore(folder)
        _levels(chain, store, folder, size_pyramid, factor, 1, fetched=fetched)
        store.close()
    finally:
        if _chain is None:
            chain.close()
    return pyr.Pyramid(folder, size_pyramid)
