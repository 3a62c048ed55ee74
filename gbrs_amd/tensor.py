"""The alignment tensor with values on the device: the arithmetic the reference builds its models from.

``DeviceTensor`` carries the in-place operations of the reference's Sparse3DMatrix / AlignmentPropertyMatrix under their
names and signatures (emase/Sparse3DMatrix.py:220-228 reset, :314-377 multiply; emase/AlignmentPropertyMatrix.py:146-153
copy, :275-303 sum, :305-370 normalize_reads) on top of gbrs_tensor_* (gbrs_amd/csrc/tensor.hip): one float64 per stored
entry of the alignment file in HBM, every operation one or two kernel launches.

    with apm.on_device() as t:
        t.normalize_reads(axis=t.Axis.READ)
        proportions = t.sum(axis=t.Axis.READ)          # (H x L)

What differs from the reference is what its sparse containers do behind the arithmetic:
  * normalize_reads on the LOCUS, GROUP and HAPLOGROUP axes eliminates the entries whose value is 0 first, as the reference
    does; such an entry stays 0 from then on (reset() included) and leaves nnz().  The structure itself never changes:
    values(h) always lines up with apm.indices[h], live(h) tells the eliminated entries apart.
  * multiply never eliminates.  (The reference's products with a locus vector and with another tensor go through scipy
    products that keep no zero result.)
  * a live entry over a zero sum raises FloatingPointError and is left unchanged, every other read is normalised.
  * the genes are part of the structure a tensor shares with its copies: a `grouping_mat` that differs from the genes in
    force replaces them for the copies too.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from enum import IntEnum

import numpy as np

from . import _lib

_FORM_LOCUS, _FORM_READ, _FORM_READ_HAP, _FORM_HAP_LOCUS = 1, 2, 3, 4


class Axis(IntEnum):
    LOCUS = 0
    HAPLOTYPE = 1
    READ = 2
    GROUP = 3
    HAPLOGROUP = 4


def groups_from_relation(grouping_mat, num_loci):
    """The genes of a locus x locus relation like the reference's t2t_mat (EMfactory.py:48-59): a list of member lists,
    ascending, one per block with more than one locus.  `grouping_mat` is a scipy sparse matrix (anything with tocoo()) or
    a dense array.  RuntimeError when it is not a block relation - reflexive, symmetric and transitive - for then the
    reference's normaliser is not a sum over the read's entries of one gene."""
    if hasattr(grouping_mat, 'tocoo'):
        coo = grouping_mat.tocoo()
        shape, keep = tuple(coo.shape), np.asarray(coo.data) != 0
        i, j = np.asarray(coo.row, dtype=np.int64)[keep], np.asarray(coo.col, dtype=np.int64)[keep]
    else:
        dense = np.asarray(grouping_mat)
        shape = dense.shape
        i, j = (x.astype(np.int64) for x in np.nonzero(dense)) if dense.ndim == 2 else (None, None)
    if shape != (num_loci, num_loci):
        raise RuntimeError(f'The grouping matrix must be {num_loci} x {num_loci}, not {shape}.')
    pairs = np.unique(i * num_loci + j)                   # (a pair stored twice counts once)
    i, j = pairs // num_loci, pairs % num_loci
    label = np.full(num_loci, num_loci, dtype=np.int64)
    np.minimum.at(label, i, j)                            # the smallest locus a locus is related to names its block
    size = np.bincount(label[label < num_loci], minlength=num_loci)
    row_nnz = np.bincount(i, minlength=num_loci)
    block = (np.bincount(i[i == j], minlength=num_loci) == 1).all() and (label[i] == label[j]).all() \
        and (row_nnz == size[np.minimum(label, num_loci - 1)]).all()
    if not block:
        raise RuntimeError('The grouping matrix is not a block relation between loci (every locus related to itself, '
                           'and to exactly the loci of its own gene).')
    order = np.argsort(label, kind='stable')
    cuts = np.flatnonzero(np.diff(label[order])) + 1
    return [g.tolist() for g in np.split(order, cuts) if len(g) > 1]


def multiply_form(multiplier, axis, shape):
    """(form of gbrs_tensor_multiply, C-contiguous float64 multiplier) of a multiply(multiplier, axis) on a tensor of
    `shape` = (L, H, R), by the rules of Sparse3DMatrix.multiply (Sparse3DMatrix.py:322-364)."""
    if hasattr(multiplier, 'tocoo'):
        raise NotImplementedError('multiply with a sparse (reads x loci) multiplier')
    m = np.asarray(multiplier, dtype=np.float64)
    L, H, R = shape
    if m.ndim == 1:
        if axis == 0:
            raise NotImplementedError('multiply with a 1-D multiplier on axis 0: the method is not yet implemented '
                                      'for the axis.')
        form, want = {1: (_FORM_LOCUS, (L,)), 2: (_FORM_READ, (R,))}.get(axis, (None, None))
    elif m.ndim == 2:
        if axis == 1:
            raise NotImplementedError('multiply with a (reads x loci) multiplier on axis 1')
        form, want = {0: (_FORM_READ_HAP, (R, H)), 2: (_FORM_HAP_LOCUS, (H, L))}.get(axis, (None, None))
    else:
        raise RuntimeError('The multiplier should be 1, 2 dimensional numpy array or a Sparse3DMatrix object.')
    if form is None:
        raise RuntimeError('The axis should be 0, 1, or 2.')
    if m.shape != want:
        raise RuntimeError(f'The multiplier of axis {int(axis)} must have the shape {want}, not {m.shape}.')
    return form, np.ascontiguousarray(m)


def genes_for(axis, grouping_mat, own_groups, num_loci):
    """The genes normalize_reads(axis, grouping_mat) sums over, as member lists: those of `grouping_mat` when one is
    given, else the tensor's own groups.  None for the axes that need none."""
    if axis not in tuple(Axis):
        raise RuntimeError('The axis should be 0, 1, 2, or 3.')
    if axis not in (Axis.GROUP, Axis.HAPLOGROUP):
        return None
    if grouping_mat is not None:
        return groups_from_relation(grouping_mat, num_loci)
    if own_groups is None:
        raise RuntimeError('Group information matrix is missing.')
    return own_groups


class DeviceTensor:
    Axis = Axis

    def __init__(self, apm, device=0):
        """Structure, stored values (ones when the file carries none), count and groups of an AlignmentPropertyMatrix; a
        pending haplotype mask is applied to the host arrays first."""
        self._h = C.c_void_p()
        apm.apply_haplotype_mask()
        L, H, R = apm.shape
        self.shape = (L, H, R)
        self.num_loci, self.num_haplotypes, self.num_reads = L, H, R
        self.device = int(device)
        self._sizes = [len(ix) for ix in apm.indices]
        lib = _lib.load()
        indptr = [np.ascontiguousarray(p, dtype=np.uint32) for p in apm.indptr]
        indices = [np.ascontiguousarray(i, dtype=np.uint32) for i in apm.indices]
        values = None if apm.values is None else [np.ascontiguousarray(v, dtype=np.float64) for v in apm.values]
        count = None if apm.count is None else np.ascontiguousarray(apm.count, dtype=np.float64)
        _lib.check(lib.gbrs_tensor_create(R, L, H, _lib.ptr_table(indptr), _lib.ptr_table(indices),
                                          None if values is None else _lib.ptr_table(values), _lib.ptr(count),
                                          self.device, C.byref(self._h)))
        self._root = self            # the tensor whose structure this one shares; it keeps the genes in force
        self._genes = None           # canonical form of the groups on the device (None: every locus its own gene)
        self._own_groups = None
        if apm.groups is not None:
            self._own_groups = self._canonical([list(map(int, g)) for g in apm.groups])
            self._set_groups(self._own_groups)

    # ---- plumbing --------------------------------------------------------------------------------------------------
    @staticmethod
    def _canonical(groups):
        return tuple(sorted(tuple(sorted(set(g))) for g in groups if len(set(g)) > 1))     # (a gene of one locus is the default)

    def _handle(self):
        if not self._h:
            raise RuntimeError('The tensor has been closed.')
        return self._h

    def _set_groups(self, genes):
        if self._root._genes == genes:
            return
        ptr = np.concatenate(([0], np.cumsum([len(g) for g in genes]))).astype(np.int64)
        mem = np.array([l for g in genes for l in g], dtype=np.int64)
        _lib.check(_lib.load().gbrs_tensor_set_groups(self._handle(), len(genes), _lib.ptr(ptr), _lib.ptr(mem)))
        self._root._genes = genes

    def close(self):
        if self._h:
            _lib.load().gbrs_tensor_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001 - interpreter shutdown
            pass

    # ---- the reference's in-place arithmetic -------------------------------------------------------------------------
    def reset(self):
        _lib.check(_lib.load().gbrs_tensor_reset(self._handle()))

    def multiply(self, multiplier, axis=None):
        lib = _lib.load()
        if isinstance(multiplier, DeviceTensor):
            if multiplier._root is not self._root:
                raise NotImplementedError('multiply with a tensor of another structure (only a copy() of the same tensor)')
            _lib.check(lib.gbrs_tensor_multiply_tensor(self._handle(), multiplier._handle()))
            return
        form, m = multiply_form(multiplier, axis, self.shape)
        _lib.check(lib.gbrs_tensor_multiply(self._handle(), form, _lib.ptr(m), m.size))

    def normalize_reads(self, axis, grouping_mat=None):
        genes = genes_for(axis, grouping_mat, self._own_groups, self.num_loci)
        self._handle()
        if genes is not None:
            self._set_groups(self._canonical(genes))
        _lib.check(_lib.load().gbrs_tensor_normalize(self._handle(), int(axis)))

    def sum(self, axis):
        lib = _lib.load()
        L, H, R = self.shape
        if axis == Axis.READ:
            out = np.empty((H, L), dtype=np.float64)
            _lib.check(lib.gbrs_tensor_sum_reads(self._handle(), _lib.ptr(out)))
            return out
        if axis == Axis.LOCUS:
            out = np.empty((R, H), dtype=np.float64)
            _lib.check(lib.gbrs_tensor_sum_loci(self._handle(), _lib.ptr(out)))
            return out
        if axis == Axis.HAPLOTYPE:
            raise NotImplementedError('sum(HAPLOTYPE): the sparse (reads x loci) sum over the haplotypes')
        raise RuntimeError('The axis should be 0, 1, or 2.')

    def copy(self, shallow=False):
        """A second value array on the same structure (shared on the device, not copied)."""
        c = object.__new__(DeviceTensor)
        c.__dict__.update(self.__dict__)
        c._h = C.c_void_p()
        _lib.check(_lib.load().gbrs_tensor_copy(self._handle(), C.byref(c._h)))
        return c

    # ---- what the host can look at -----------------------------------------------------------------------------------
    def _fetch(self, h, want_live):
        if not 0 <= int(h) < self.num_haplotypes:
            raise IndexError(f'haplotype {h} out of range')
        n = self._sizes[int(h)]
        val = np.empty(n, dtype=np.float64)
        live = np.empty(n, dtype=np.uint8) if want_live else None
        _lib.check(_lib.load().gbrs_tensor_values(self._handle(), int(h), _lib.ptr(val), _lib.ptr(live), n))
        return val, live

    def values(self, h):
        """The values of haplotype h, lined up with apm.indices[h]; 0 at an eliminated entry."""
        return self._fetch(h, False)[0]

    def live(self, h):
        """bool mask over apm.indices[h]: False where normalize_reads has eliminated the entry."""
        return self._fetch(h, True)[1].astype(bool)

    def set_values(self, h, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        if not 0 <= int(h) < self.num_haplotypes or v.shape != (self._sizes[int(h)],):
            raise RuntimeError('The values do not match the stored entries of the haplotype.')
        _lib.check(_lib.load().gbrs_tensor_set_values(self._handle(), int(h), _lib.ptr(v), v.size))

    def nnz(self, per_haplotype=False):
        """Live entries (all stored entries until a normalize_reads eliminates some)."""
        out = np.zeros(self.num_haplotypes, dtype=np.uint64)
        _lib.check(_lib.load().gbrs_tensor_nnz(self._handle(), _lib.ptr(out)))
        return out if per_haplotype else int(out.sum())

    # ---- the rest of the reference's interface -------------------------------------------------------------------------
    def _not_here(name):       # noqa: N805
        def method(self, *a, **kw):
            raise NotImplementedError(f'{name} is not available on the device tensor')
        method.__name__ = name
        return method

    add = _not_here('add')
    __add__ = _not_here('__add__')
    __sub__ = _not_here('__sub__')
    __mul__ = _not_here('__mul__')
    bundle = _not_here('bundle')
    get_cross_section = _not_here('get_cross_section')
    del _not_here
