"""Host-side mirror of the reference interface for the hot path, batch-shaped.

Reference (crate decaf377 v0.10.1)              here (one call = one batch)
  Encoding(pub [u8; 32])                          Encoding(array[n, 32] u8)
  Encoding::vartime_decompress()                  Encoding.vartime_decompress() -> (Element, status)
  Element::vartime_compress()                     Element.vartime_compress() -> Encoding
  Element::encode_to_curve(&Fq)                   Element.encode_to_curve(Fq) -> Encoding
  Element::hash_to_curve(&Fq, &Fq)                Element.hash_to_curve(Fq, Fq) -> Encoding
  Element::GENERATOR * Fr                         Element.generator_mul(Fr) -> Encoding
  FixedBase tables over any Elements (ark-ec)     FixedBases(Element).vartime_multiscalar_mul(Fr) -> Encoding
  element * Fr  (Encoding in, Encoding out)       Encoding.scalar_mul(Fr) -> (Encoding, status)
  Fq::sqrt_ratio_zeta(&num, &den)                 Fq.sqrt_ratio_zeta(num, den) -> (was_square, Fq)
  EncodingError::InvalidEncoding                  status byte 1 (0 = Ok) / EncodingError when raised

Arrays may be numpy (host path: the library stages through HBM) or torch CUDA tensors (device
path: no copies, launched on torch's current stream).  torch is plumbing only: device memory
and streams.  There is no CPU implementation behind these classes."""
import ctypes

import numpy as np

from . import _native


class EncodingError(ValueError):
    """src/error.rs:1-5. `InvalidEncoding` is reported per element as status 1."""


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _torch_stream(dev):
    """torch's current stream on `dev`, as the hipStream_t argument of a device-pointer call."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _rows(a):
    if a.ndim < 1:
        raise ValueError("expected a [n, k] array of packed records")
    return int(a.shape[0])


# row layouts of the packed records (trailing shape, element kind): the native code reads and writes
# n * (that many bytes) unconditionally, so every array is checked against these before a call
ENC = ((32,), "u8")          # Encoding / Fq / Fr byte strings
ELEM = ((16,), "u64")        # Element: X, Y, Z, T as 4 Montgomery limbs each
FQM = ((4,), "u64")          # Fq as 4 Montgomery limbs
AFF = ((8,), "u64")          # affine x, y
FLAG = ((), "u8")            # one status / flag byte per element
SQRT_ROOT = {"ark": 0, "arkworks": 0, "min_curve": 1}
# D377_TUNE_* keys of d377_ctx_set_tuning (include/decaf377_amd.h, "Developer interface")
TUNE_KEYS = {"small_max": 0, "decompress_chunked_min": 1, "fb_wide": 2, "fb_k": 3, "affine_blocks_per_cu": 4, "msm_window": 5,
             "msm_seg": 6, "msm_small_max": 7, "msm_slices": 8, "msm_red": 9, "msm_skip": 10, "msm_chunked_sums": 11,
             "msm_enc_chunked_min": 12, "chunk_per_lane": 13, "msm_tiny_max": 14, "tiny_max": 15, "msm_sort_packed": 16}
SHARD_OPS = {"sqrt_ratio_zeta": 0, "decompress": 1, "compress": 2, "roundtrip": 3, "scalar_mul_base": 4,
             "scalar_mul_var": 5, "encode_to_curve": 6, "hash_to_curve": 7, "scalar_mul_var_element": 8,
             "scalar_mul_base_element": 9}


def _check(a, spec, n, what, device=None):
    """Raises ValueError unless `a` is a contiguous-able [n, *tail] array of the right element type
    (and, for torch tensors, lives on `device`)."""
    tail, kind = spec
    shape = tuple(int(x) for x in a.shape)
    if shape != (n,) + tail:
        raise ValueError("%s: expected shape %s, got %s" % (what, (n,) + tail, shape))
    if _is_torch(a):
        import torch
        ok = a.dtype == torch.uint8 if kind == "u8" else a.dtype in (torch.int64, torch.uint64)
        if device is not None and a.device != device:
            raise ValueError("%s: tensor on %s, expected %s" % (what, a.device, device))
    else:
        ok = a.dtype == np.uint8 if kind == "u8" else a.dtype in (np.uint64, np.int64)
    if not ok:
        raise ValueError("%s: expected %s elements, got %s" % (what, "uint8" if kind == "u8" else "uint64/int64", a.dtype))


# ---- what the batched sums of Context and FixedBases share: every argument rule once, on numpy arrays for the host route
# (dev None) and on tensors for the resident route (dev: the device of the context the call runs on)
def _cuda_device(ctx, *arrays):
    """The device of the first tensor among `arrays` that lives on a device of `ctx`, or None: which calls take the resident
    forms.  Every other input -- numpy, CPU tensors, tensors on a GPU the context does not own -- keeps the host path."""
    return next((a.device for a in arrays if _is_torch(a) and a.device.type == "cuda" and a.device.index in ctx.device_ids), None)


def _on_device(dev, a):
    """`a` as a contiguous tensor on `dev` (a numpy array or a tensor that lives elsewhere is copied there)."""
    import torch
    if not _is_torch(a):
        a = np.ascontiguousarray(a)
        a = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a)
    return a.detach().to(dev).contiguous()


def _staged(dev, a):
    """`a` where the route reads it: a contiguous numpy array (a CPU tensor shares its memory with it, any other tensor is
    copied to the host), or a contiguous tensor on `dev`."""
    if dev is not None:
        return _on_device(dev, a)
    return np.ascontiguousarray(a.detach().cpu().numpy() if _is_torch(a) else a)


def _is_u8(a):
    if _is_torch(a):
        import torch
        return a.dtype == torch.uint8
    return a.dtype == np.uint8


def _u64_dtypes():
    import torch
    return (torch.int64, torch.uint64)


def _ptr(a):
    """The void* argument for an array of either kind, which the caller keeps alive through the call; None is NULL."""
    if a is None:
        return None
    return ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def _index(dev, index, what, arg, rule="must be an [n, t] integer array"):
    """`index` as a contiguous [n, t] int32 array of the route's kind.  Any integer type is accepted and converted; one that
    holds a value outside 32 bits is refused (on the resident route one synchronising reduction, for wider types only)."""
    if dev is None:
        idx = np.asarray(index.detach().cpu().numpy() if _is_torch(index) else index)
        integer, i32 = idx.dtype.kind in "iu", np.int32
    else:
        import torch
        idx = index if _is_torch(index) else torch.from_numpy(np.ascontiguousarray(index))
        integer, i32 = idx.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64), torch.int32
    if idx.ndim != 2 or not integer:
        raise ValueError("%s: %s %s" % (what, arg, rule))
    if dev is not None:
        idx = idx.detach().to(dev)
    if idx.dtype != i32:
        if 0 not in idx.shape and (int(idx.min()) < -(1 << 31) or int(idx.max()) >= (1 << 31)):
            raise ValueError("%s: %s does not fit 32 bits" % (what, arg))
        idx = idx.astype(i32) if dev is None else idx.to(i32)
    return np.ascontiguousarray(idx) if dev is None else idx.contiguous()


def _records(dev, a, spec, n, t, mismatch, what):
    """[n * t, k] or [n, t, k] records that go with an [n, t] index -> the staged [n * t, k] array, checked against `spec`;
    `mismatch`: the caller's text for an [n, t, k] array whose first two dimensions are not the index's."""
    a = _staged(dev, a)
    if a.ndim == 3:
        if tuple(a.shape[:2]) != (n, t):
            raise ValueError(mismatch)
        a = a.reshape((n * t,) + spec[0])
    _check(a, spec, n * t, what)
    return a


def _out_specs(n, elements, status_rows=None):
    """(row layout, rows) of the outputs of a sums call, in the C order: enc, xyzt with elements, status for Encodings."""
    return [(ENC, n)] + ([(ELEM, n)] if elements else []) + ([(FLAG, status_rows)] if status_rows is not None else [])


def _outputs(what, dev, n, elements, status_rows=None, outs=None):
    """The outputs of a sums call: enc [n, 32], xyzt [n, 16] with elements, status [status_rows] for Encodings -- numpy arrays on
    the host route; on the resident route tensors allocated on `dev`, or the caller's `outs` in that order, checked like inputs."""
    if dev is None:
        res = [np.zeros((n, 32), np.uint8)] + ([np.zeros((n, 16), np.uint64)] if elements else [])
        return res + [np.zeros((status_rows,), np.uint8)] if status_rows is not None else res
    import torch
    specs = _out_specs(n, elements, status_rows)
    if outs is None:
        return [torch.empty((rows,) + tail, dtype=torch.uint8 if k == "u8" else torch.int64, device=dev) for (tail, k), rows in specs]
    if len(outs) != len(specs):
        raise ValueError("%s: %d output arrays expected" % (what, len(specs)))
    for a, (spec, rows) in zip(outs, specs):
        if not _is_torch(a):
            raise ValueError(what + ": outs must be tensors on the inputs' device")
        _check(a, spec, rows, what + " output", dev)
        if not a.is_contiguous():
            raise ValueError(what + " output must be contiguous")
    return list(outs)


def _out_ptrs(res, elements):
    """The output pointers in the C order enc, xyzt, [status]: xyzt is NULL without elements."""
    ptrs = [_ptr(a) for a in res]
    if not elements:
        ptrs.insert(1, None)
    return ptrs


def _results(res, dev, arrays, verdict=None, into=None):
    """What a sums call returns: its outputs, the verdict tensor of an unchecked resident call appended; one array alone is
    returned bare.  The host route's arrays go to the device of the first tensor among the caller's `arrays`, when there is
    one (Element records as int64 there), and from there into the caller's own tensors `into`, when it gave some."""
    if dev is None:
        for given in arrays:
            if _is_torch(given):
                import torch
                res = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(given.device) for a in res]
                if into is not None:
                    for o, r in zip(into, res):
                        o.copy_(r)
                    res = list(into)
                break
    if verdict is not None:
        res = list(res) + [verdict]
    return tuple(res) if len(res) > 1 else res[0]


def _verdict_tensor(dev, n):
    """The [2] int64 record a resident call writes; a call of no sums enqueues nothing, so its record is made here."""
    import torch
    verdict = torch.zeros((2,), dtype=torch.int64, device=dev)
    if n == 0:
        verdict[1] = -1
    return verdict


def _refused_index(symbol, arg, first, value, t, noun):
    """The native library's text for the first refused index of an [n, t] array, restated for the resident routes: there the
    library has made no refusal whose text could be read.  tests/test_resident_sums_gpu.py::
    test_python_checks_the_indices_before_any_launch compares the two texts."""
    return _native.error(-2, "%s: %s[%d] = %d (sum %d, term %d) is neither -1 nor a %s" % (symbol, arg, first, value, first // t, first % t, noun))


class Context:
    """Owns the device tables and scratch for one or more GPUs (d377_ctx)."""

    def __init__(self, device_ids=None, comb_bits=0, comb_lazy=False):
        """comb_bits: width of the fixed-base comb, 0 = the library's default (23) or 18 / 21 / 23 (0.24 / 1.6 / 5.9 GB per
        device); comb_lazy: build it on the first fixed-base call instead of now (d377_ctx_create_ex) -- a context that
        never multiplies by the generator then holds 0.73 GB per device instead of 6.7."""
        self._lib = _native.load()
        self._h = ctypes.c_void_p()
        if device_ids is None:
            ids, n = None, 0
        else:
            ids, n = (ctypes.c_int * len(device_ids))(*device_ids), len(device_ids)
        if comb_bits == 0 and not comb_lazy:
            _native.check(self._lib.d377_ctx_create(ids, n, ctypes.byref(self._h)))
        else:
            opts = _native.CtxOpts(ctypes.sizeof(_native.CtxOpts), int(comb_bits), 1 if comb_lazy else 0)
            _native.check(self._lib.d377_ctx_create_ex(ids, n, ctypes.byref(opts), ctypes.byref(self._h)))
        self.device_ids = [self._lib.d377_ctx_device_id(self._h, i)
                           for i in range(self._lib.d377_ctx_num_devices(self._h))]

    def invariant_failures(self, dev=0):
        """(checks compiled in?, count): d377_ctx_invariant_failures -- the -DD377_CHECK_INVARIANTS build's
        counterpart of the reference's debug assertions (src/min_curve/element.rs:104-110)."""
        c = ctypes.c_uint64(0)
        rc = self._lib.d377_ctx_invariant_failures(self._h, dev, ctypes.byref(c))
        if rc < 0:
            _native.check(rc)
        return rc == 1, int(c.value)

    def comb_info(self, dev=0):
        """(width in bits, built yet?, table bytes) of the device's fixed-base comb: d377_ctx_comb_info."""
        a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_uint64(0)
        _native.check(self._lib.d377_ctx_comb_info(self._h, dev, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return int(a.value), bool(b.value), int(c.value)

    def chunk_residency(self, dev=0):
        """(lane sets per CU, largest residency of a set-claiming kernel per CU, LDS padding in bytes):
        d377_ctx_chunk_residency -- what d377_ctx_create verified with the occupancy query."""
        a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _native.check(self._lib.d377_ctx_chunk_residency(self._h, dev, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def peer_access(self, a, b):
        """d377_ctx_peer_access: 2 = distinct GPUs with peer access enabled, 1 = the same GPU listed twice, 0 = none."""
        return int(self._lib.d377_ctx_peer_access(self._h, a, b))

    def health(self, dev=0):
        """(lane sets claimed now, workgroups that waited > 0.25 s for a set, workgroups that gave up): d377_ctx_health."""
        a, b, c = ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _native.check(self._lib.d377_ctx_health(self._h, dev, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def reset_scratch(self, dev=0):
        """Frees lane sets leaked by a launch that died (d377_ctx_reset_scratch) -> how many it freed."""
        a = ctypes.c_int(0)
        _native.check(self._lib.d377_ctx_reset_scratch(self._h, dev, ctypes.byref(a)))
        return int(a.value)

    def starved_counter(self, dev=0):
        """The gave-up counter as a 1-element uint32 CUDA tensor that aliases the library's word
        (d377_ctx_starved_counter_dev): a `_dev` caller copies it on its stream before and after a call and compares
        once the stream has been synchronised -- a call whose kernels starved has left output records unwritten."""
        import torch
        p = ctypes.c_void_p()
        _native.check(self._lib.d377_ctx_starved_counter_dev(self._h, dev, ctypes.byref(p)))

        class _Word:
            __cuda_array_interface__ = {"shape": (1,), "typestr": "<i4", "data": (int(p.value), False), "version": 2}
        return torch.as_tensor(_Word(), device=torch.device("cuda", self.device_ids[dev]))

    def _debug_poison_pool(self, dev=0, sets=-1):
        _native.check(self._lib.d377_debug_poison_pool(self._h, dev, sets))

    def set_tuning(self, key, value=None):
        """d377_ctx_set_tuning: developer override of one launch rule (TUNE_KEYS); value None restores the built-in rule."""
        _native.check(self._lib.d377_ctx_set_tuning(self._h, TUNE_KEYS[key], -1 if value is None else int(value)))

    def get_tuning(self, key):
        v = ctypes.c_int64(0)
        _native.check(self._lib.d377_ctx_get_tuning(self._h, TUNE_KEYS[key], ctypes.byref(v)))
        return None if v.value < 0 else int(v.value)

    def tuning(self, **kv):
        """Context manager: the given overrides for the calls made inside, the previous values afterwards."""
        ctx = self

        class _Scope:
            def __enter__(self):
                self.old = {k: ctx.get_tuning(k) for k in kv}
                for k, v in kv.items():
                    ctx.set_tuning(k, v)
                return ctx

            def __exit__(self, *exc):
                for k, v in self.old.items():
                    ctx.set_tuning(k, v)
                return False

        return _Scope()

    def fixed_bases(self, points, comb_bits=16):
        """Registers 1 <= m <= 64 fixed bases ([m, 16] u64 Element records, numpy or torch) and builds one comb per base on
        every device of the context (d377_fixed_bases_create): comb_bits 8 / 12 / 16 / 18 = 0.53 / 5.5 / 67 / 235 MB per base.
        Returns a FixedBases; it keeps this context alive and is closed before it."""
        return FixedBases(points, comb_bits=comb_bits, ctx=self)

    def fixed_bases_long(self, points, comb_bits=12):
        """Registers 1 <= m <= 4096 fixed bases (d377_fixed_bases_create_long): fixed_bases with room for the generators of a
        vector commitment -- 4096 bases are 2.2 GB at 8 bits and 22.5 GB at 12 on every device.  The FixedBases' msm cuts every
        sum into segments that fill the chip (FixedBases.msm_long, which also takes a short registration)."""
        return FixedBases(points, comb_bits=comb_bits, ctx=self, long=True)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            for fb in list(getattr(self, "_fixed", ())):          # handles first: d377_fixed_bases_destroy before d377_ctx_destroy
                fb.close()
            self._lib.d377_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing ---------------------------------------------------------------------------
    def _dev_index(self, dev):
        if dev.type != "cuda":
            raise _native.NativeError("torch tensors must live on the GPU (there is no CPU path)")
        if dev.index not in self.device_ids:
            raise _native.NativeError("tensor on cuda:%s but context owns %s" % (dev.index, self.device_ids))
        return self.device_ids.index(dev.index)

    def _run(self, name, ins, in_specs, out_specs, outs=None, pre=(), sharded_op=None, in_slots=None):
        """ins: input arrays (specs in `in_specs`); out_specs: row layouts of the outputs.  Host or
        device path by the type of the first input; `pre` = extra integer arguments that precede the
        buffers in the C signature; `outs` lets a caller reuse output arrays (checked like inputs).
        sharded_op: run through d377_batch_sharded_dev (HBM-resident batch split over the context's GPUs).
        in_slots: input-pointer parameters of the C signature when some are unused by this call (passed NULL)."""
        n = _rows(ins[0])
        np_dt = {"u8": np.uint8, "u64": np.uint64}
        if _is_torch(ins[0]):
            import torch
            dev = ins[0].device
            di = self._dev_index(dev)
            for a, spec in zip(ins, in_specs):
                _check(a, spec, n, name + " input", dev)
            tdt = {"u8": torch.uint8, "u64": torch.int64}
            ins = [t.contiguous() for t in ins]
            if outs is None:
                outs = [torch.empty((n,) + tail, dtype=tdt[k], device=dev) for tail, k in out_specs]
            else:
                if len(outs) != len(out_specs):
                    raise ValueError("%s: expected %d output arrays" % (name, len(out_specs)))
                for a, spec in zip(outs, out_specs):
                    _check(a, spec, n, name + " output", dev)
                    if not a.is_contiguous():
                        raise ValueError("%s output must be contiguous" % name)
            stream = torch.cuda.current_stream(dev).cuda_stream
            bufs = [ctypes.c_void_p(t.data_ptr()) for t in ins]
            obufs = [ctypes.c_void_p(t.data_ptr()) for t in outs]
            if sharded_op is not None:
                bufs += [None] * (2 - len(bufs))
                obufs += [None] * (2 - len(obufs))
                _native.check(self._lib.d377_batch_sharded_dev(self._h, di, ctypes.c_void_p(stream), sharded_op,
                                                               bufs[0], bufs[1], ctypes.c_size_t(n), obufs[0], obufs[1]))
                return outs
            bufs += [None] * ((in_slots or len(bufs)) - len(bufs))
            args = [self._h, di, ctypes.c_void_p(stream)] + list(pre) + bufs + [ctypes.c_size_t(n)] + obufs
            _native.check(getattr(self._lib, name + "_dev")(*args))
            return outs
        if sharded_op is not None:
            raise ValueError("the sharded path takes torch CUDA tensors (host arrays are sharded by the host path)")
        ins = [np.ascontiguousarray(a) for a in ins]
        for a, spec in zip(ins, in_specs):
            _check(a, spec, n, name + " input")
        if outs is None:
            # fresh arrays of this size are mmap'ed anew on every call and fault their pages in during the copy back;
            # a caller that cares passes `outs` it allocated once (tools/host_path_bench.py: 2^20 round trips 7-9 ms vs 4.8 ms)
            outs = [np.empty((n,) + tail, dtype=np_dt[k]) for tail, k in out_specs]
        else:
            if len(outs) != len(out_specs):
                raise ValueError("%s: expected %d output arrays" % (name, len(out_specs)))
            for a, spec in zip(outs, out_specs):
                _check(a, spec, n, name + " output")
                if not a.flags["C_CONTIGUOUS"]:
                    raise ValueError("%s output must be contiguous" % name)
        args = [self._h] + list(pre) + [a.ctypes.data_as(ctypes.c_void_p) for a in ins]
        args += [None] * ((in_slots or len(ins)) - len(ins)) + [ctypes.c_size_t(n)]
        args += [a.ctypes.data_as(ctypes.c_void_p) for a in outs]
        _native.check(getattr(self._lib, name)(*args))
        return outs

    # -- the batch operations (C ABI names) ---------------------------------------------------
    def sqrt_ratio_zeta(self, num32, den32, outs=None, root="ark"):
        """root: "ark" (Sarkar tables, src/ark_curve/invsqrt.rs:75-166) or "min_curve" (Tonelli-Shanks
        seeded with 11^m, src/min_curve/invsqrt.rs:11-95): same flags, root negated about half the time."""
        return self._run("d377_batch_sqrt_ratio_zeta_ex", [num32, den32], [ENC, ENC], [ENC, FLAG], outs,
                         pre=(ctypes.c_int(SQRT_ROOT[root]),))

    def decompress(self, enc32, outs=None):
        return self._run("d377_batch_decompress", [enc32], [ENC], [ELEM, FLAG], outs)

    def compress(self, xyzt, outs=None):
        return self._run("d377_batch_compress", [xyzt], [ELEM], [ENC], outs)[0]

    def roundtrip(self, enc32, outs=None):
        return self._run("d377_batch_roundtrip", [enc32], [ENC], [ENC, FLAG], outs)

    def scalar_mul_base(self, scalar32, outs=None):
        return self._run("d377_batch_scalar_mul_base", [scalar32], [ENC], [ENC], outs)[0]

    def scalar_mul_var(self, enc32, scalar32, outs=None):
        return self._run("d377_batch_scalar_mul_var", [enc32, scalar32], [ENC, ENC], [ENC, FLAG], outs)

    def encode_to_curve(self, fq32, outs=None):
        return self._run("d377_batch_encode_to_curve", [fq32], [ENC], [ENC], outs)[0]

    def hash_to_curve(self, r1_32, r2_32, outs=None):
        return self._run("d377_batch_hash_to_curve", [r1_32, r2_32], [ENC, ENC], [ENC], outs)[0]

    # The reference's own signatures: Elements in and out, no encoding step (src/min_curve/ops.rs:89-95,
    # src/min_curve/element.rs:163-181, 190-244).  A scalar multiplication returns some extended representative
    # of the reference's group element: compare with eq() or through compress().
    def scalar_mul_var_element(self, p_xyzt, scalar32, outs=None):
        return self._run("d377_batch_scalar_mul_var_element", [p_xyzt, scalar32], [ELEM, ENC], [ELEM], outs)[0]

    def scalar_mul_base_element(self, scalar32, outs=None):
        return self._run("d377_batch_scalar_mul_base_element", [scalar32], [ENC], [ELEM], outs)[0]

    def compress_to_field(self, p_xyzt, outs=None):
        """Element::vartime_compress_to_field -> [n, 4] u64 Montgomery limbs of s."""
        return self._run("d377_batch_compress_to_field", [p_xyzt], [ELEM], [FQM], outs)[0]

    def encode_to_curve_element(self, fq32, outs=None):
        return self._run("d377_batch_encode_to_curve_element", [fq32], [ENC], [ELEM], outs)[0]

    def hash_to_curve_element(self, r1_32, r2_32, outs=None):
        return self._run("d377_batch_hash_to_curve_element", [r1_32, r2_32], [ENC, ENC], [ELEM], outs)[0]

    def add(self, p_xyzt, q_xyzt, outs=None):
        return self._run("d377_batch_add", [p_xyzt, q_xyzt], [ELEM, ELEM], [ELEM], outs)[0]

    def sub(self, p_xyzt, q_xyzt, outs=None):
        """Element - Element = self + other.neg() (src/min_curve/ops.rs:43-87)."""
        return self._run("d377_batch_sub", [p_xyzt, q_xyzt], [ELEM, ELEM], [ELEM], outs)[0]

    def double(self, p_xyzt, outs=None):
        return self._run("d377_batch_double", [p_xyzt], [ELEM], [ELEM], outs)[0]

    def eq(self, p_xyzt, q_xyzt, outs=None):
        return self._run("d377_batch_eq", [p_xyzt, q_xyzt], [ELEM, ELEM], [FLAG], outs)[0]

    def neg(self, p_xyzt, outs=None):
        return self._run("d377_batch_neg", [p_xyzt], [ELEM], [ELEM], outs)[0]

    def is_identity(self, p_xyzt, outs=None):
        return self._run("d377_batch_is_identity", [p_xyzt], [ELEM], [FLAG], outs)[0]

    def sharded(self, op, in0, in1=None, outs=None):
        """d377_batch_sharded_dev: an HBM-resident batch (torch CUDA tensors on one device of this context)
        split into contiguous slices over all the context's GPUs by peer copies over xGMI.  op is one of
        SHARD_OPS; inputs and outputs are those of the method of the same name."""
        specs = {"sqrt_ratio_zeta": ([ENC, ENC], [ENC, FLAG]), "decompress": ([ENC], [ELEM, FLAG]),
                 "compress": ([ELEM], [ENC]), "roundtrip": ([ENC], [ENC, FLAG]), "scalar_mul_base": ([ENC], [ENC]),
                 "scalar_mul_var": ([ENC, ENC], [ENC, FLAG]), "encode_to_curve": ([ENC], [ENC]),
                 "hash_to_curve": ([ENC, ENC], [ENC]), "scalar_mul_var_element": ([ELEM, ENC], [ELEM]),
                 "scalar_mul_base_element": ([ENC], [ELEM])}[op]
        ins = [in0] if in1 is None else [in0, in1]
        if len(ins) != len(specs[0]):
            raise ValueError("%s takes %d input arrays" % (op, len(specs[0])))
        return self._run("d377_batch_sharded_dev:" + op, ins, specs[0], specs[1], outs, sharded_op=SHARD_OPS[op])

    def identity(self):
        """Element::IDENTITY as one [16] u64 record (src/min_curve/element.rs:53-58)."""
        out = np.zeros(16, np.uint64)
        self._lib.d377_identity(out.ctypes.data_as(ctypes.c_void_p))
        return out

    def generator(self):
        """Element::GENERATOR as one [16] u64 record (src/min_curve/element.rs:61-81)."""
        out = np.zeros(16, np.uint64)
        self._lib.d377_generator(out.ctypes.data_as(ctypes.c_void_p))
        return out


    # -- Fr byte handling ---------------------------------------------------------------------------
    def fr_from_le_bytes_mod_order(self, bytes32, outs=None):
        """Fr::from_le_bytes_mod_order on [n, 32] byte strings -> canonical [n, 32] (src/fields/fr.rs:82-94)."""
        return self._run("d377_batch_fr_from_le_bytes_mod_order", [bytes32], [ENC], [ENC], outs)[0]

    def fr_from_bytes_checked(self, bytes32, outs=None):
        """Fr::from_bytes_checked (src/fields/fr.rs:100-107) -> ([n, 32], status[n]); a rejected record is all-zero."""
        return self._run("d377_batch_fr_from_bytes_checked", [bytes32], [ENC], [ENC, FLAG], outs)

    def fr_op(self, op, a32, b32=None, outs=None):
        """Fr add/sub/mul (binary) and square/neg/inverse (unary) on [n, 32] little-endian scalars
        (src/fields/fr/u64/wrapper.rs:76-108): inputs reduced mod r, outputs canonical -> (out [n, 32], status [n]);
        status 1 (and a zero record) only for inverse(0).  numpy arrays or torch CUDA tensors."""
        code = self.FQ_OPS[op]
        binary = code <= 2
        if binary != (b32 is not None):
            raise ValueError("fr_op %s takes %s" % (op, "two operands" if binary else "one operand"))
        ins = [a32, b32] if binary else [a32]
        return self._run("d377_batch_fr_op", ins, [ENC] * len(ins), [ENC, FLAG], outs, pre=(ctypes.c_int(code),), in_slots=2)

    def fr_from_wide_bytes(self, data):
        """Fr::from_le_bytes_mod_order on [n, 48|64] byte strings -> canonical [n, 32] (src/fields/fr.rs:82-94)."""
        return self._wide("d377_batch_fr_from_wide_bytes", data)

    # -- Fq on in-memory elements (4 Montgomery u64 limbs) ------------------------------------------
    FQ_OPS = {"add": 0, "sub": 1, "mul": 2, "square": 3, "neg": 4, "inverse": 5}

    def fq_op(self, op, a, b=None, outs=None):
        """Fq add/sub/mul (binary) and square/neg/inverse (unary) on [n, 4] u64 Montgomery records
        (src/fields/fq/u64/wrapper.rs:99-132) -> (out [n, 4], status [n]); status 1 only for inverse(0).
        numpy arrays (host path) or torch CUDA tensors (device path)."""
        code = self.FQ_OPS[op]
        binary = code <= 2
        if binary and b is None:
            raise ValueError("fq_op %s takes two operands" % op)
        ins = [a, b] if binary else [a]
        if not _is_torch(a):                                     # host arrays: any integer layout of n x 4 limbs
            ins = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in ins]
            if binary and ins[1].shape[0] != ins[0].shape[0]:
                raise ValueError("fq_op: operands have %d and %d rows" % (ins[0].shape[0], ins[1].shape[0]))
        return self._run("d377_batch_fq_op", ins, [FQM] * len(ins), [FQM, FLAG], outs, pre=(ctypes.c_int(code),), in_slots=2)

    def fq_from_bytes_checked(self, bytes32, outs=None):
        """Fq::from_bytes_checked (src/fields/fq.rs:108-115) -> ([n, 4] u64, status[n])."""
        return self._run("d377_batch_fq_from_bytes_checked", [bytes32], [ENC], [FQM, FLAG], outs)

    def fq_to_bytes(self, a, outs=None):
        """Fq::to_bytes_le on [n, 4] u64 Montgomery records -> [n, 32] u8."""
        return self._run("d377_batch_fq_to_bytes", [a], [FQM], [ENC], outs)[0]

    # -- wide byte strings and affine normalisation -----------------------------------------------
    def _wide(self, name, data):
        if data.ndim != 2 or int(data.shape[1]) not in (48, 64):
            raise ValueError("%s: expected [n, 48] or [n, 64] byte strings, got shape %s" % (name, tuple(data.shape)))
        n, length = int(data.shape[0]), int(data.shape[1])
        _check(data, ((length,), "u8"), n, name + " input")
        if _is_torch(data):
            import torch
            dev = data.device
            self._dev_index(dev)
            out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _native.check(getattr(self._lib, name + "_dev")(self._h, self.device_ids.index(dev.index), stream,
                                                            ctypes.c_void_p(data.contiguous().data_ptr()),
                                                            ctypes.c_size_t(length), ctypes.c_size_t(n),
                                                            ctypes.c_void_p(out.data_ptr())))
            return out
        data = np.ascontiguousarray(data, dtype=np.uint8)
        out = np.zeros((n, 32), np.uint8)
        _native.check(getattr(self._lib, name)(self._h, data.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(length),
                                               ctypes.c_size_t(n), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def fq_from_wide_bytes(self, data):
        """Fq::from_le_bytes_mod_order on [n, 48|64] byte strings -> canonical [n, 32]."""
        return self._wide("d377_batch_fq_from_wide_bytes", data)

    def encode_to_curve_wide(self, data):
        """encode_to_curve(Fq::from_le_bytes_mod_order(bytes)) for [n, 48|64] byte strings."""
        return self._wide("d377_batch_encode_to_curve_wide", data)

    def to_affine(self, xyzt, outs=None):
        """CurveGroup::normalize_batch: [n, 16] Elements -> [n, 8] (x, y Montgomery limbs)."""
        return self._run("d377_batch_to_affine", [xyzt], [ELEM], [AFF], outs)[0]

    # -- multi-scalar multiplication -------------------------------------------------------------
    def msm_small(self, points, scalar32, m, outs=None, elements=False):
        """n independent multiscalar sums of m terms each (d377_batch_msm_small[_encoded]): Element::vartime_multiscalar_mul
        (src/ark_curve/element/projective.rs:99-117) in the shape of the reference's own test, a 3-term sum per case
        (tests/operations.rs:44-60), many at once.  points: [n * m, 16] u64 Elements or [n * m, 32] u8 Encodings, scalar32:
        [n * m, 32], term-major within a sum; 1 <= m <= 8.  Returns enc [n, 32] for Elements, (enc, status [n * m]) for
        Encodings (an invalid Encoding is reported and left out of its sum); with elements=True the sums also come back as
        Element records, what the reference's function returns: (enc, xyzt [n, 16]) / (enc, xyzt, status), in d377_msm's
        order.  outs: the same tuple of preallocated arrays."""
        return self._sums_of_m("msm_small", ("d377_batch_msm_small", "d377_batch_msm_small_encoded"),
                               ("d377_batch_msm_small_dev", "d377_batch_msm_small_encoded_dev"), points, scalar32, m, outs, elements,
                               stage_foreign=False)

    def msm_long(self, points, scalar32, m, outs=None, elements=False):
        """n independent multiscalar sums of m terms each, 1 <= m <= 4096 (d377_batch_msm_long[_encoded]): msm_small's sums
        at medium length -- every sum cut into Straus chains of at most 8 terms whose partial sums are folded on the device.
        points: [n * m, 16] u64 Elements or [n * m, 32] u8 Encodings (detected by the row width, as msm_small does),
        scalar32: [n * m, 32], term-major within a sum.  Returns what msm_small returns: enc [n, 32] for Elements, (enc,
        status [n * m]) for Encodings; with elements=True (enc, xyzt [n, 16]) / (enc, xyzt, status).  outs: the same tuple
        of preallocated arrays.  Tensors on a device of the context take d377_batch_long_msm[_encoded]_resident on torch's
        current stream: no copy, no synchronisation, the results on that device.  numpy arrays keep the host-pointer call,
        and tensors on a GPU the context does not own are staged through host memory (the results come back on the points'
        device).  For ONE long sum use msm()."""
        return self._sums_of_m("msm_long", ("d377_batch_msm_long", "d377_batch_msm_long_encoded"),
                               ("d377_batch_long_msm_resident", "d377_batch_long_msm_encoded_resident"), points, scalar32, m, outs, elements)

    def _launch(self, dev, host_symbol, device_symbol, *args):
        """One native call of a sums family: `host_symbol`(ctx, *args) on the host route (dev None), else
        `device_symbol`(ctx, device index, torch's current stream on dev, *args)."""
        if dev is None:
            _native.check(getattr(self._lib, host_symbol)(self._h, *args))
        else:
            _native.check(getattr(self._lib, device_symbol)(self._h, self._dev_index(dev), _torch_stream(dev), *args))

    def _sums_of_m(self, what, host_names, device_names, points, scalar32, m, outs, elements, extra=(), stage_foreign=True):
        """What msm_small, msm_long and msm_buckets share: n sums of m terms, on the host or on the device by where the points
        live; `extra`: the call's own arguments between n and the outputs.  stage_foreign: a tensor on a GPU the context does
        not own is staged through host memory (msm_long, msm_buckets); without it every tensor takes the device call, which
        refuses such a tensor (msm_small)."""
        m = int(m)
        if points.ndim != 2 or int(points.shape[1]) not in (16, 32):
            raise ValueError("%s: " % what + "points must be [n * m, 16] Elements or [n * m, 32] Encodings")
        encoded = int(points.shape[1]) == 32
        terms = _rows(points)
        if m < 1 or terms % m:
            raise ValueError("%s: " % what + "the number of points must be a multiple of m")
        n = terms // m
        return self._sums(what, host_names, device_names, points, scalar32, encoded, terms, n, outs, elements,
                          lambda dev: (ctypes.c_size_t(m), ctypes.c_size_t(n), *extra), stage_foreign)

    def _sums(self, what, host_names, device_names, points, scalar32, encoded, terms, n, outs, elements, mid, stage_foreign=True):
        """The staging, the outputs and the launch of n sums over `terms` rows of `points`, Encodings if `encoded`, for
        _sums_of_m and msm_ragged; mid(dev): the call's own arguments between the scalars and the outputs, for the route
        taken (dev None: the host form)."""
        tdev = points.device if _is_torch(points) else None
        _check(points, ENC if encoded else ELEM, terms, what + " points")
        _check(scalar32, ENC, terms, what + " scalars", tdev)
        status_rows = terms if encoded else None
        specs = _out_specs(n, elements, status_rows) if outs is not None else None
        if outs is not None and len(outs) != len(specs):
            raise ValueError("%s: " % what + "%d output arrays expected" % len(specs))
        dev = tdev if tdev is not None and (not stage_foreign or _cuda_device(self, points) is not None) else None
        if dev is not None:                                      # no copy, no synchronisation, torch's current stream
            self._dev_index(dev)                                 # (raises for a tensor that is on no device of the context)
            pts, sc = points.detach().contiguous(), scalar32.detach().contiguous()
            res = _outputs(what, dev, n, elements, status_rows, outs)
        else:
            if tdev is not None:
                if tdev.type != "cuda":
                    self._dev_index(tdev)                        # (raises: there is no CPU path for tensors)
                if outs is not None:
                    for a, (spec, rows) in zip(outs, specs):
                        _check(a, spec, rows, what + " output", tdev)
            pts, sc = _staged(None, points), _staged(None, scalar32)
            res = outs if outs is not None and tdev is None else _outputs(what, None, n, elements, status_rows)
        self._launch(dev, host_names[encoded], device_names[encoded], _ptr(pts), _ptr(sc), *mid(dev), *_out_ptrs(res, elements))
        return _results(res, dev, (points,), into=outs)

    def msm_buckets(self, points, scalar32, m, outs=None, elements=False, window_bits=0):
        """n independent multiscalar sums of m terms each, 1 <= m <= 2^20, by the bucket method
        (d377_batch_bucket_msm[_encoded], include/decaf377_amd_bucket_sums.h): the sums of a pass share one run of msm()'s
        sort / span / bucket pipeline under a composite bucket key.  Arguments, results and routing are msm_long's: points
        [n * m, 16] u64 Elements or [n * m, 32] u8 Encodings, scalar32 [n * m, 32], term-major; tensors on a device of the
        context take the resident form on torch's current stream (one eager call of a shape before capturing it in a graph).
        window_bits: 0 = the library's width rule; 4 .. 16 forces the window width (a developer and test knob)."""
        return self._sums_of_m("msm_buckets", ("d377_batch_bucket_msm", "d377_batch_bucket_msm_encoded"),
                               ("d377_batch_bucket_msm_resident", "d377_batch_bucket_msm_encoded_resident"), points, scalar32, m, outs,
                               elements, extra=(ctypes.c_int(int(window_bits)),))

    def msm_buckets_plan(self, n, m, window_bits=0, dev=0):
        """The plan of msm_buckets for n sums of m terms on device `dev` of the context (d377_bucket_msm_plan) ->
        {"window_bits", "sums_per_pass", "passes", "workspace_bytes"}."""
        c = ctypes.c_int(0)
        spp, passes, ws = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _native.check(self._lib.d377_bucket_msm_plan(self._h, int(dev), ctypes.c_size_t(int(n)), ctypes.c_size_t(int(m)), int(window_bits),
                                                     ctypes.byref(c), ctypes.byref(spp), ctypes.byref(passes), ctypes.byref(ws)))
        return {"window_bits": c.value, "sums_per_pass": spp.value, "passes": passes.value, "workspace_bytes": ws.value}

    @staticmethod
    def _offsets(what, offsets):
        """`offsets` as a contiguous uint64 array on the host: n + 1 values that start at 0 and never decrease."""
        off = np.asarray(offsets.detach().cpu().numpy() if _is_torch(offsets) else offsets)
        if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
            raise ValueError(what + ": offsets must be n + 1 integers")
        if off.dtype.kind == "i" and (off < 0).any():
            raise ValueError(what + ": offsets must not be negative")
        off = np.ascontiguousarray(off, dtype=np.uint64)
        if off[0] != 0 or (off[1:] < off[:-1]).any():
            raise ValueError(what + ": offsets must start at 0 and never decrease")
        return off

    def msm_ragged(self, points, scalar32, offsets, outs=None, elements=False, window_bits=0, offsets_dev=None):
        """n independent multiscalar sums of ANY length each, 0 .. 2^20 terms per sum, by the bucket method
        (d377_batch_ragged_msm[_encoded], include/decaf377_amd_ragged_sums.h): sum i is the terms offsets[i] ..
        offsets[i + 1] - 1 of points [terms, 16] u64 Elements or [terms, 32] u8 Encodings and scalar32 [terms, 32].  offsets:
        n + 1 integers on the host (anything numpy turns into int64 or uint64), offsets[0] == 0, never decreasing,
        offsets[n] == terms.  Results, outs and routing are msm_buckets's; status has offsets[n] rows; an empty sum gives the
        all-zero Encoding.  Tensors on a device of the context take the resident form on torch's current stream (one eager
        call of a shape before capturing it in a graph).  offsets_dev: the same n + 1 values as a uint64 / int64 tensor on
        that device, which the kernels read.  When it is None THIS METHOD ALLOCATES A TENSOR AND COPIES THE OFFSETS TO THE
        DEVICE, which a stream capture does not allow: a caller who captures a graph passes its own.  Nothing checks that
        offsets_dev holds the values of offsets; if it does not, the sums are wrong (memory stays safe).
        window_bits: 0 = the library's width rule on the mean length; 4 .. 16 forces the window width."""
        what = "msm_ragged"
        off = self._offsets(what, offsets)
        n = int(off.size) - 1
        if points.ndim != 2 or int(points.shape[1]) not in (16, 32):
            raise ValueError(what + ": points must be [terms, 16] Elements or [terms, 32] Encodings")
        encoded, terms = int(points.shape[1]) == 32, _rows(points)
        if terms != int(off[n]):
            raise ValueError(what + ": offsets[n] = %d, but there are %d points" % (int(off[n]), terms))
        held = []                                                # keeps the uploaded offsets alive through the call

        def mid(dev):
            args = [_ptr(off)]
            if dev is not None:
                od = offsets_dev
                if od is None:
                    od = _on_device(dev, off)
                elif not (_is_torch(od) and od.device == dev and od.dtype in _u64_dtypes() and tuple(od.shape) == (n + 1,)
                          and od.is_contiguous()):
                    raise ValueError(what + ": offsets_dev must be a contiguous [n + 1] uint64/int64 tensor on the points' device")
                held.append(od)
                args.append(_ptr(od))
            return (*args, ctypes.c_size_t(n), ctypes.c_int(int(window_bits)))

        return self._sums(what, ("d377_batch_ragged_msm", "d377_batch_ragged_msm_encoded"),
                          ("d377_batch_ragged_msm_resident", "d377_batch_ragged_msm_encoded_resident"), points, scalar32, encoded, terms, n, outs,
                          elements, mid)

    def msm_ragged_plan(self, offsets, window_bits=0, dev=0):
        """The plan of msm_ragged for the sums `offsets` delimits on device `dev` of the context (d377_ragged_msm_plan) ->
        {"window_bits", "passes", "max_sums_per_pass", "max_points_per_pass", "workspace_bytes"}."""
        off = self._offsets("msm_ragged_plan", offsets)
        c = ctypes.c_int(0)
        v = [ctypes.c_uint64(0) for _ in range(4)]
        _native.check(self._lib.d377_ragged_msm_plan(self._h, int(dev), _ptr(off), ctypes.c_size_t(int(off.size) - 1), int(window_bits),
                                                     ctypes.byref(c), *(ctypes.byref(x) for x in v)))
        return {"window_bits": c.value, "passes": v[0].value, "max_sums_per_pass": v[1].value, "max_points_per_pass": v[2].value,
                "workspace_bytes": v[3].value}

    def msm_segmented(self, points, scalar32, offsets, outs=None, elements=False, offsets_dev=None):
        """n independent multiscalar sums of ANY length each, 0 .. 2^20 terms per sum, by Straus chains
        (d377_batch_segmented_msm[_encoded], include/decaf377_amd_segmented_sums.h): msm_ragged's arguments without
        window_bits, its Encodings and statuses byte for byte, and msm_long's cut of every sum into chains of at most 8 terms
        -- the call for MANY SHORT sums of unequal length (msm_segmented_plan's "advised_route", which msm_by_offsets
        follows).  Element records are some representative of the sums, not msm_ragged's bytes.  Routing is msm_ragged's:
        tensors on a device of the context take the resident form on torch's current stream (one eager call of a shape
        before capturing it in a graph).  offsets_dev: the same n + 1 values as a uint64 / int64 tensor on that device, which
        the kernels read.  When it is None THIS METHOD ALLOCATES A TENSOR AND COPIES THE OFFSETS TO THE DEVICE, which a
        stream capture does not allow: a caller who captures a graph passes its own.  Nothing checks that offsets_dev holds
        the values of offsets; if it does not, the sums are wrong (memory stays safe)."""
        what = "msm_segmented"
        off = self._offsets(what, offsets)
        n = int(off.size) - 1
        if points.ndim != 2 or int(points.shape[1]) not in (16, 32):
            raise ValueError(what + ": points must be [terms, 16] Elements or [terms, 32] Encodings")
        encoded, terms = int(points.shape[1]) == 32, _rows(points)
        if terms != int(off[n]):
            raise ValueError(what + ": offsets[n] = %d, but there are %d points" % (int(off[n]), terms))
        held = []                                                # keeps the uploaded offsets alive through the call

        def mid(dev):
            args = [_ptr(off)]
            if dev is not None:
                od = offsets_dev
                if od is None:
                    od = _on_device(dev, off)
                elif not (_is_torch(od) and od.device == dev and od.dtype in _u64_dtypes() and tuple(od.shape) == (n + 1,)
                          and od.is_contiguous()):
                    raise ValueError(what + ": offsets_dev must be a contiguous [n + 1] uint64/int64 tensor on the points' device")
                held.append(od)
                args.append(_ptr(od))
            return (*args, ctypes.c_size_t(n))

        return self._sums(what, ("d377_batch_segmented_msm", "d377_batch_segmented_msm_encoded"),
                          ("d377_batch_segmented_msm_resident", "d377_batch_segmented_msm_encoded_resident"), points, scalar32, encoded, terms,
                          n, outs, elements, mid)

    def msm_segmented_plan(self, offsets, dev=0):
        """The plan of msm_segmented for the sums `offsets` delimits on device `dev` of the context (d377_segmented_msm_plan)
        -> {"chain_slots", "chains", "fold_levels", "max_slots_per_chain", "scratch_bytes", "advised_route"}; advised_route
        is "chains" (this call) or "buckets" (msm_ragged)."""
        off = self._offsets("msm_segmented_plan", offsets)
        u = [ctypes.c_uint64(0) for _ in range(3)]
        c = [ctypes.c_int(0) for _ in range(3)]
        _native.check(self._lib.d377_segmented_msm_plan(self._h, int(dev), _ptr(off), ctypes.c_size_t(int(off.size) - 1), ctypes.byref(u[0]),
                                                        ctypes.byref(u[1]), ctypes.byref(c[0]), ctypes.byref(c[1]), ctypes.byref(u[2]),
                                                        ctypes.byref(c[2])))
        return {"chain_slots": u[0].value, "chains": u[1].value, "fold_levels": c[0].value, "max_slots_per_chain": c[1].value,
                "scratch_bytes": u[2].value, "advised_route": ("chains", "buckets")[c[2].value]}

    def msm_by_offsets(self, points, scalar32, offsets, outs=None, elements=False, offsets_dev=None, route="auto"):
        """n sums delimited by offsets on the route that suits their lengths: the whole call goes to msm_segmented
        (route="chains") or to msm_ragged with the library's window rule (route="buckets"); "auto" takes
        msm_segmented_plan's advised_route for the device the points live on (device 0 of the context for host arrays).
        The Encodings and statuses do not depend on the route; Element records are some representative of the same sums."""
        if route not in ("auto", "chains", "buckets"):
            raise ValueError('msm_by_offsets: route must be "auto", "chains" or "buckets"')
        if route == "auto":
            dev = _cuda_device(self, points) if _is_torch(points) else None
            route = self.msm_segmented_plan(offsets, dev=self._dev_index(dev) if dev is not None else 0)["advised_route"]
        call = self.msm_segmented if route == "chains" else self.msm_ragged
        return call(points, scalar32, offsets, outs=outs, elements=elements, offsets_dev=offsets_dev)

    def msm_long_indexed(self, pool, point_index, scalar32, m, elements=False, check_indices=True, outs=None):
        """n sums of m terms that name their points in a shared pool (d377_batch_long_msm_indexed):

            out[i] = sum over j < m of scalars[i m + j] * pool[point_index[i, j]]

        pool: [pool_count, 16] u64 Elements (a record with Z = 0 is the identity).  point_index: [n, m] int32 (int64 is
        accepted and range-checked), each 0 .. pool_count-1, repeats allowed, or -1 for an absent term -- which costs as
        much as a present one, so m is the longest sum's length; 1 <= m <= 4096 and m must equal point_index's second
        dimension.  scalar32: [n * m, 32] or [n, m, 32] u8.  -> enc [n, 32] u8, or (enc, xyzt [n, 16]) with
        elements=True.  Any other index raises NativeError and nothing is computed.
        Routing is FixedBases.msm_indexed's: numpy arrays, CPU tensors and tensors on a GPU the context does not own take
        the host-pointer call (sliced over the devices of a multi-GPU context, the pool sent to each).  When the pool, the
        indices or the scalars are a tensor on a device of the context, the call runs on that one device: it is
        d377_batch_long_msm_indexed_resident on torch's current stream (the other arguments are copied there if they live
        elsewhere) and the results are allocated there.  check_indices=True first reduces the indices on the device and
        reads the result -- the call's one synchronisation -- so that a refused index raises as above with no sum launched.
        check_indices=False is fully asynchronous: the verdict tensor ([2] int64: the count of refused indices, the first
        position or -1 = UINT64_MAX) is appended to the returned tuple, and a refused index has contributed nothing to its
        sum.  outs: preallocated contiguous tensors on that device in the order of the result, without the verdict; the
        host route allocates its own arrays and refuses outs with ValueError."""
        what = "msm_long_indexed"
        m = int(m)
        if pool.ndim != 2 or int(pool.shape[1]) != 16:
            raise ValueError(what + ": pool must be [pool_count, 16] Elements")
        pool_count = _rows(pool)
        _check(pool, ELEM, pool_count, what + " pool")
        dev = _cuda_device(self, pool, point_index, scalar32)
        if dev is None and outs is not None:
            raise ValueError(what + ": outs goes with tensors on a device of the context")
        idx = _index(dev, point_index, what, "point_index", "must be an [n, m] integer array")
        n = int(idx.shape[0])
        if int(idx.shape[1]) != m:
            raise ValueError(what + ": point_index must be [n, m]")
        pl = _staged(dev, pool)
        sc = _records(dev, scalar32, ENC, n, m, what + ": scalars [n, m, 32] must match point_index [n, m]", what + " scalars")
        verdict = None
        if dev is not None and check_indices:
            flat = idx.reshape(-1)
            bad = ((flat != -1) & ((flat < 0) | (flat >= pool_count))).nonzero()
            if bad.numel():                                      # (the one synchronisation)
                first = int(bad[0])
                raise _refused_index("d377_batch_long_msm_indexed", "point_index", first, int(flat[first]), m,
                                     "record 0 .. %d of the pool" % (pool_count - 1))
        elif dev is not None:
            verdict = _verdict_tensor(dev, n)
        res = _outputs(what, dev, n, elements, outs=outs)
        self._launch(dev, "d377_batch_long_msm_indexed", "d377_batch_long_msm_indexed_resident", _ptr(pl), ctypes.c_size_t(pool_count),
                     _ptr(idx), _ptr(sc), ctypes.c_size_t(m), ctypes.c_size_t(n), *_out_ptrs(res, elements),
                     *(() if dev is None else (_ptr(verdict),)))
        return _results(res, dev, (pool, point_index, scalar32), verdict)

    def msm(self, points, scalar32, encoded=None):
        """Element::vartime_multiscalar_mul (src/ark_curve/element/projective.rs:99-117).
        points: [n, 16] u64 Elements or [n, 32] u8 Encodings (detected by the row width).
        Returns (enc[32] u8, xyzt[16] u64, status[n] or None)."""
        n = _rows(points)
        if points.ndim != 2 or int(points.shape[1]) not in (16, 32):
            raise ValueError("msm: points must be [n, 16] Elements or [n, 32] Encodings")
        if encoded is None:
            encoded = int(points.shape[1]) == 32
        # the reference zips scalars with points (projective.rs:99-117); a length mismatch is a caller bug here
        _check(points, ENC if encoded else ELEM, n, "msm points")
        _check(scalar32, ENC, n, "msm scalars", points.device if _is_torch(points) else None)
        if _is_torch(points):
            import torch
            dev = points.device
            self._dev_index(dev)
            pts, sc = points.contiguous(), scalar32.contiguous()
            enc = torch.empty((32,), dtype=torch.uint8, device=dev)
            xyzt = torch.empty((16,), dtype=torch.int64, device=dev)
            st = torch.empty((max(n, 1),), dtype=torch.uint8, device=dev) if encoded else None
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            di = self.device_ids.index(dev.index)
            p = lambda t: ctypes.c_void_p(t.data_ptr())
            if encoded:
                _native.check(self._lib.d377_msm_encoded_dev(self._h, di, stream, p(pts), p(sc), ctypes.c_size_t(n),
                                                             p(enc), p(xyzt), p(st)))
                return enc, xyzt, st[:n]
            _native.check(self._lib.d377_msm_dev(self._h, di, stream, p(pts), p(sc), ctypes.c_size_t(n), p(enc), p(xyzt)))
            return enc, xyzt, None
        pts = np.ascontiguousarray(points)
        sc = np.ascontiguousarray(scalar32)
        enc = np.zeros(32, np.uint8)
        xyzt = np.zeros(16, np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        if encoded:
            st = np.zeros(max(n, 1), np.uint8)
            _native.check(self._lib.d377_msm_encoded(self._h, p(pts), p(sc), ctypes.c_size_t(n), p(enc), p(xyzt), p(st)))
            return enc, xyzt, st[:n]
        _native.check(self._lib.d377_msm(self._h, p(pts), p(sc), ctypes.c_size_t(n), p(enc), p(xyzt)))
        return enc, xyzt, None

    @staticmethod
    def _short_scalars(scalars, n, device):
        """The scalars of msm_short as n packed little-endian records -> (contiguous array or tensor, bytes per record).
        [n, 8] or [n, 16] uint8, or uint64 of shape [n] / [n, 2] (little-endian words; int64 tensors count as uint64)."""
        torch_in = _is_torch(scalars)
        if device is not None and (not torch_in or scalars.device != device):
            raise ValueError("msm_short scalars: expected a tensor on %s" % (device,))
        if device is None and torch_in:
            raise ValueError("msm_short scalars: a tensor goes with points on a device of the context")
        shape = tuple(int(x) for x in scalars.shape)
        if torch_in:
            import torch
            is_u8, is_u64 = scalars.dtype == torch.uint8, scalars.dtype in (torch.int64, torch.uint64)
        else:
            is_u8, is_u64 = scalars.dtype == np.uint8, scalars.dtype in (np.uint64, np.int64)
        if is_u8 and shape in ((n, 8), (n, 16)):
            nbytes = shape[1]
        elif is_u64 and shape in ((n,), (n, 1), (n, 2)):
            nbytes = 16 if shape == (n, 2) else 8
        else:
            raise ValueError("msm_short scalars: expected [%d, 8] or [%d, 16] uint8, or uint64 of shape [%d] or [%d, 2], got %s %s"
                             % (n, n, n, n, scalars.dtype, shape))
        return (scalars.contiguous() if torch_in else np.ascontiguousarray(scalars)), nbytes

    def msm_short(self, points, scalars, encoded=None):
        """msm() over scalars known to be short (d377_msm_short[_encoded], include/decaf377_amd_short_msm.h): the weights of a
        batch verification (128 bits), amounts (u64 / u128).  The bytes returned are those of msm() on the same scalars
        zero-extended to 32 bytes, from 5 or 9 windows of digits instead of 16.
        points: [n, 16] u64 Elements or [n, 32] u8 Encodings (detected by the row width).
        scalars: [n, 8] or [n, 16] uint8, or uint64 of shape [n] / [n, 2] (little-endian words).
        Tensors on a device of the context take the _dev form on torch's current stream (one eager call of a shape before
        capturing it in a graph).  Returns (enc[32] u8, xyzt[16] u64, status[n] or None)."""
        n = _rows(points)
        if points.ndim != 2 or int(points.shape[1]) not in (16, 32):
            raise ValueError("msm_short: points must be [n, 16] Elements or [n, 32] Encodings")
        if encoded is None:
            encoded = int(points.shape[1]) == 32
        _check(points, ENC if encoded else ELEM, n, "msm_short points")
        sz, nb = ctypes.c_size_t(n), None
        if _is_torch(points):
            import torch
            dev = points.device
            di = self._dev_index(dev)
            sc, nb = self._short_scalars(scalars, n, dev)
            pts = points.contiguous()
            enc = torch.empty((32,), dtype=torch.uint8, device=dev)
            xyzt = torch.empty((16,), dtype=torch.int64, device=dev)
            st = torch.empty((max(n, 1),), dtype=torch.uint8, device=dev) if encoded else None
            stream = _torch_stream(dev)
            p = lambda t: ctypes.c_void_p(t.data_ptr())
            if encoded:
                _native.check(self._lib.d377_msm_short_encoded_dev(self._h, di, stream, p(pts), p(sc), nb, sz, p(enc), p(xyzt), p(st)))
                return enc, xyzt, st[:n]
            _native.check(self._lib.d377_msm_short_dev(self._h, di, stream, p(pts), p(sc), nb, sz, p(enc), p(xyzt)))
            return enc, xyzt, None
        sc, nb = self._short_scalars(scalars, n, None)
        pts = np.ascontiguousarray(points)
        enc = np.zeros(32, np.uint8)
        xyzt = np.zeros(16, np.uint64)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        if encoded:
            st = np.zeros(max(n, 1), np.uint8)
            _native.check(self._lib.d377_msm_short_encoded(self._h, p(pts), p(sc), nb, sz, p(enc), p(xyzt), p(st)))
            return enc, xyzt, st[:n]
        _native.check(self._lib.d377_msm_short(self._h, p(pts), p(sc), nb, sz, p(enc), p(xyzt)))
        return enc, xyzt, None

    def msm_short_plan(self, n, scalar_bytes, dev=0):
        """The plan of msm_short for n terms of 8- or 16-byte scalars on device `dev` of the context (d377_msm_short_plan) ->
        {"window_bits", "windows", "workspace_bytes"}."""
        c, w, ws = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_uint64(0)
        _native.check(self._lib.d377_msm_short_plan(self._h, int(dev), ctypes.c_size_t(int(n)), int(scalar_bytes), ctypes.byref(c),
                                                    ctypes.byref(w), ctypes.byref(ws)))
        return {"window_bits": c.value, "windows": w.value, "workspace_bytes": ws.value}

    def sum_elements(self, xyzt):
        """Sum of m Element records held in HBM -> (enc[32], xyzt[16]); used to combine the
        per-rank partial sums of a sharded MSM."""
        import torch
        m = _rows(xyzt)
        _check(xyzt, ELEM, m, "sum_elements input")
        dev = xyzt.device
        self._dev_index(dev)
        enc = torch.empty((32,), dtype=torch.uint8, device=dev)
        out = torch.empty((16,), dtype=torch.int64, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _native.check(self._lib.d377_sum_elements_dev(self._h, self.device_ids.index(dev.index), stream,
                                                      ctypes.c_void_p(xyzt.contiguous().data_ptr()), ctypes.c_size_t(m),
                                                      ctypes.c_void_p(enc.data_ptr()), ctypes.c_void_p(out.data_ptr())))
        return enc, out


class FixedBases:
    """Fixed-base combs for caller-chosen points (d377_fixed_bases_create / d377_batch_fixed_msm): the reference's
    Element works with ark-ec's FixedBase window tables (src/ark_curve/element.rs:22-38); here one comb per base lives on
    every device of the context and one call computes n sums

        out[i] = scalars[i m] * B_0 + ... + scalars[i m + m - 1] * B_{m-1}

    points: an Element batch or an [m, 16] u64 array of Element records (numpy or torch; read once, at creation).
    comb_bits: 8, 12, 16 or 18.  ctx: the Context (default_context() if None); the FixedBases keeps it alive, and
    Context.close() closes every FixedBases of the context first.  Usable as a context manager.
    long: register with d377_fixed_bases_create_long, up to 4096 bases instead of 64 (Context.fixed_bases_long)."""

    def __init__(self, points, comb_bits=16, ctx=None, long=False):
        if isinstance(points, Element):
            ctx = ctx or points.ctx
            points = points.data
        self.ctx = ctx or default_context()
        if _is_torch(points):
            points = points.detach().cpu().numpy()
        pts = np.ascontiguousarray(np.asarray(points).view(np.uint64) if np.asarray(points).dtype == np.int64 else points)
        if pts.ndim != 2 or pts.shape[1] != 16 or pts.dtype != np.uint64:
            raise ValueError("FixedBases: points must be [m, 16] u64 Element records")
        self._lib = self.ctx._lib
        self._h = 0
        if not self.ctx._h:
            raise _native.NativeError("FixedBases: the context is closed")
        h = ctypes.c_int64(0)
        create = self._lib.d377_fixed_bases_create_long if long else self._lib.d377_fixed_bases_create
        _native.check(create(self.ctx._h, pts.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(pts.shape[0]), int(comb_bits), ctypes.byref(h)))
        self._h = int(h.value)
        if not hasattr(self.ctx, "_fixed"):
            import weakref
            self.ctx._fixed = weakref.WeakSet()
        self.ctx._fixed.add(self)
        self.m, self.comb_bits, self.table_bytes = self.info()

    def info(self):
        """(m, comb width in bits, table bytes per device): d377_fixed_bases_info."""
        m, b, t = ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_uint64(0)
        _native.check(self._lib.d377_fixed_bases_info(self.ctx._h, self._live(), ctypes.byref(m), ctypes.byref(b), ctypes.byref(t)))
        return int(m.value), int(b.value), int(t.value)

    def _live(self):
        if not self._h:
            raise _native.NativeError("FixedBases: the handle is closed")
        return self._h

    def msm(self, scalar32, elements=False):
        """n sums over the registered bases: scalar32 [n * m, 32] u8, term-major within a sum (any 32 bytes, reduced mod r)
        -> enc [n, 32] u8, or (enc, xyzt [n, 16]) with elements=True.  A numpy array or a CPU tensor takes the host-pointer
        call, and so does a tensor on a GPU the context does not own (staged through host memory, the results back on its
        device); a tensor on a device of the context takes d377_batch_fixed_msm_resident on torch's current stream, with
        no copy and no synchronisation, and the results are allocated on its device -- on that ONE device: a multi-GPU
        context slices host arrays over its devices, never a resident tensor."""
        return self._dense("d377_batch_fixed_msm", "FixedBases.msm", scalar32, elements)

    def msm_long(self, scalar32, elements=False):
        """msm with every sum cut into segments of consecutive bases, one GPU lane per segment, where that fills the chip
        (d377_batch_fixed_long_msm; long_plan shows the cut): few sums over many bases.  The same arguments and results as
        msm, on a short or a long registration; msm on more than 64 bases is this call."""
        return self._dense("d377_batch_fixed_long_msm", "FixedBases.msm_long", scalar32, elements)

    def long_plan(self, n, dev=0):
        """(segments per sum, bases per segment) of msm_long for the slice of n sums that device `dev` of the context gets:
        d377_fixed_long_msm_plan."""
        g, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _native.check(self._lib.d377_fixed_long_msm_plan(self.ctx._h, self._live(), ctypes.c_size_t(n), int(dev), ctypes.byref(g), ctypes.byref(b)))
        return int(g.value), int(b.value)

    def _dense(self, symbol, what, scalar32, elements):
        h = self._live()
        dev = _cuda_device(self.ctx, scalar32)
        sc = _staged(dev, scalar32)
        terms = _rows(sc)
        if terms % self.m:
            raise ValueError("%s: the number of scalars must be a multiple of m = %d" % (what, self.m))
        n = terms // self.m
        _check(sc, ENC, terms, what + " scalars")
        res = _outputs(what, dev, n, elements)
        self.ctx._launch(dev, symbol, symbol + "_resident", h, _ptr(sc), ctypes.c_size_t(n), *_out_ptrs(res, elements))
        return _results(res, dev, (scalar32,))

    def _verdict(self, dev, idx, check_indices, symbol):
        """The index verdict of a resident call (None on the host route, where the library refuses by itself).
        check_indices=True: d377_check_base_index_resident, then the one synchronisation -- the 16-byte record is read, and on
        a refused index NativeError with the host form's text is raised before any sum is launched; returns None.
        check_indices=False: the tensor the call writes its verdict to."""
        if dev is None:
            return None
        if not check_indices:
            return _verdict_tensor(dev, int(idx.shape[0]))
        import torch
        verdict = torch.empty((2,), dtype=torch.int64, device=dev)
        self.ctx._launch(dev, None, "d377_check_base_index_resident", self._live(), _ptr(idx), ctypes.c_size_t(idx.numel()), _ptr(verdict))
        count, first = (int(x) & ((1 << 64) - 1) for x in verdict.cpu().tolist())
        if count:
            raise _refused_index(symbol, "base_index", first, int(idx.reshape(-1)[first].item()), int(idx.shape[1]),
                                 "base 0 .. %d of this registration" % (self.m - 1))
        return None

    def msm_indexed(self, base_index, scalar32, elements=False, check_indices=True, outs=None):
        """n sums of t terms that name their bases (d377_batch_fixed_msm_indexed):

            out[i] = sum over j < t of scalars[i t + j] * B_{base_index[i, j]}

        base_index: [n, t] int32 (int64 is accepted and range-checked), each 0 .. m-1 or -1 for an absent term -- which
        costs as much as a present one, so t should be the longest sum's length.  scalar32: [n * t, 32] or [n, t, 32] u8,
        term-major (any 32 bytes, reduced mod r).  -> enc [n, 32] u8, or (enc, xyzt [n, 16]) with elements=True.  An index
        outside -1 .. m-1 raises NativeError and nothing is computed.
        numpy arrays, CPU tensors and tensors on a GPU the context does not own take the host-pointer call (staged, sliced
        over the devices of a multi-GPU context).  When the scalars or the indices are a tensor on a device of the context
        the call runs on that one device: it is d377_batch_fixed_msm_indexed_resident on torch's current stream (the other argument is
        copied to that device if it lives elsewhere) and the results are allocated there.  check_indices=True first runs the
        index verdict alone and reads its 16-byte record -- the call's one synchronisation -- so that a refused index raises
        as above, with no sum launched.  check_indices=False is fully asynchronous: nothing is read, the verdict tensor
        ([2] int64: the count of refused indices, the first position or -1 = UINT64_MAX) is appended to the returned tuple,
        and a refused index has contributed nothing to its sum.  outs, a supported part of this route as of msm_small's
        and msm_long's: preallocated contiguous tensors on that device in the order of the result, without the verdict, for
        callers that keep their buffers (a captured graph, a pipeline); the host route allocates its own arrays and
        refuses outs with ValueError."""
        what = "FixedBases.msm_indexed"
        h = self._live()
        dev = _cuda_device(self.ctx, scalar32, base_index)
        if dev is None and outs is not None:
            raise ValueError(what + ": outs goes with tensors on a device of the context")
        idx = _index(dev, base_index, what, "base_index")
        n, t = (int(x) for x in idx.shape)
        sc = _records(dev, scalar32, ENC, n, t, what + ": scalars [n, t, 32] must match base_index [n, t]", what + " scalars")
        symbol = "d377_batch_fixed_msm_indexed"
        verdict = self._verdict(dev, idx, check_indices, symbol)
        res = _outputs(what, dev, n, elements, outs=outs)
        self.ctx._launch(dev, symbol, symbol + "_resident", h, _ptr(idx), _ptr(sc), ctypes.c_size_t(t), ctypes.c_size_t(n),
                         *_out_ptrs(res, elements), *(() if dev is None else (_ptr(verdict),)))
        return _results(res, dev, (scalar32, base_index), verdict)

    def msm_mixed(self, base_index, fixed_scalar32, points, var_scalar32, elements=False, check_indices=True, outs=None):
        """n mixed sums, registered bases plus variable points (d377_batch_msm_mixed[_encoded]):

            out[i] = sum over j < t of fixed[i t + j] * B_{base_index[i, j]}  +  sum over p < v of var[i v + p] * P[i v + p]

        base_index: [n, t] int32 as in msm_indexed (-1 = absent, as costly as a present term), 1 <= t <= 64.
        fixed_scalar32: [n * t, 32] or [n, t, 32] u8.  points: [n, v, 16] / [n * v, 16] u64 Element records, or [n, v, 32] /
        [n * v, 32] u8 Encodings, 1 <= v <= 8.  var_scalar32: [n * v, 32] or [n, v, 32] u8.  Scalars are any 32 bytes, reduced
        mod r.  -> enc [n, 32] u8, or (enc, xyzt [n, 16]) with elements=True; for Encodings status [n * v] u8 is appended
        (1 = invalid Encoding, that term left out of its sum): msm_small's order.  An index outside -1 .. m-1 raises
        NativeError and nothing is computed.
        numpy arrays, CPU tensors and tensors on a GPU the context does not own take the host-pointer call.  When any
        argument is a tensor on a device of the context the call runs on that one device: it is d377_batch_msm_mixed[_encoded]_resident on torch's current stream, on the device of the first such tensor
        among points, the scalars and the indices (arguments that live elsewhere are copied there), and the results are
        allocated on it.  check_indices is msm_indexed's: True reads the index verdict first, the one synchronisation, and
        raises before any sum is launched; False is fully asynchronous and appends the verdict tensor to the result; outs
        (this route only) are preallocated tensors on that device in the order of the result, without the verdict."""
        what = "FixedBases.msm_mixed"
        h = self._live()
        args = (points, var_scalar32, fixed_scalar32, base_index)
        dev = _cuda_device(self.ctx, *args)
        if dev is None and outs is not None:
            raise ValueError(what + ": outs goes with tensors on a device of the context")
        idx = _index(dev, base_index, what, "base_index")
        n, t = (int(x) for x in idx.shape)
        fs = _records(dev, fixed_scalar32, ENC, n, t, what + ": fixed scalars [n, t, 32] must match base_index [n, t]", what + " fixed scalars")
        pts = _staged(dev, points)
        if pts.ndim == 3:
            if int(pts.shape[0]) != n:
                raise ValueError(what + ": points [n, v, .] must have one row per sum")
            pts = pts.reshape(pts.shape[0] * pts.shape[1], pts.shape[2])
        encoded = _is_u8(pts)
        terms = _rows(pts)
        if n == 0 or terms % n:
            if terms or n:
                raise ValueError(what + ": the number of points must be a multiple of the number of sums")
        v = terms // n if n else 1
        _check(pts, ENC if encoded else ELEM, n * v, what + " points")
        vs = _records(dev, var_scalar32, ENC, n, v, what + ": variable scalars [n, v, 32] must match the points [n, v, .]",
                      what + " variable scalars")
        symbol = "d377_batch_msm_mixed_encoded" if encoded else "d377_batch_msm_mixed"
        verdict = self._verdict(dev, idx, check_indices, symbol)
        res = _outputs(what, dev, n, elements, n * v if encoded else None, outs)
        self.ctx._launch(dev, symbol, symbol + "_resident", h, _ptr(idx), _ptr(fs), ctypes.c_size_t(t), _ptr(pts), _ptr(vs),
                         ctypes.c_size_t(v), ctypes.c_size_t(n), *_out_ptrs(res, elements), *(() if dev is None else (_ptr(verdict),)))
        return _results(res, dev, args, verdict)

    def vartime_multiscalar_mul(self, scalars):
        """The sums' Encodings for an Fr batch (or [n * m, 32] array) of n x m scalars, term-major within a sum."""
        return Encoding(self.msm(scalars.data if isinstance(scalars, _Bytes32) else scalars), self.ctx)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _native.check(self._lib.d377_fixed_bases_destroy(self.ctx._h, self._h))
            self._h = 0
            fixed = getattr(self.ctx, "_fixed", None)
            if fixed is not None:
                fixed.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default = None


def default_context():
    global _default
    if _default is None:
        _default = Context()
    return _default


class _Bytes32:
    """A batch of 32-byte little-endian records, shape [n, 32] uint8."""

    def __init__(self, data, ctx=None):
        if not _is_torch(data):
            data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8)).reshape(-1, 32)
        self.data = data
        self.ctx = ctx

    def _ctx(self):
        return self.ctx or default_context()

    def __len__(self):
        return int(self.data.shape[0])

    def to_bytes(self):
        d = self.data.cpu().numpy() if _is_torch(self.data) else self.data
        return [bytes(r) for r in d]


class Fq(_Bytes32):
    """Batch of base-field elements given as 32 bytes, interpreted mod q like
    Fq::from_le_bytes_mod_order (src/fields/fq.rs:90-102)."""

    @staticmethod
    def sqrt_ratio_zeta(num, den, root="ark"):
        """Fq::sqrt_ratio_zeta (src/ark_curve/invsqrt.rs:75-166; root="min_curve": the min_curve backend's
        non_arkworks_sqrt_ratio_zeta, src/min_curve/invsqrt.rs:73-95) -> (was_square[n], Fq roots)."""
        r, ws = num._ctx().sqrt_ratio_zeta(num.data, den.data, root=root)
        return ws, Fq(r, num.ctx)


class Fr(_Bytes32):
    """Batch of scalars given as 32 bytes, interpreted mod r like Fr::from_le_bytes_mod_order
    (src/fields/fr.rs:82-94)."""

    def _op(self, op, other=None):
        out, st = self._ctx().fr_op(op, self.data, None if other is None else other.data)
        return Fr(out, self.ctx), st

    def __add__(self, other):
        return self._op("add", other)[0]

    def __sub__(self, other):
        return self._op("sub", other)[0]

    def __mul__(self, other):
        """Fr * Fr, or Fr * Element = Element * Fr (src/min_curve/ops.rs:89-95)."""
        if isinstance(other, Element):
            return other * self
        return self._op("mul", other)[0]

    def __neg__(self):
        return self._op("neg")[0]

    def square(self):
        return self._op("square")[0]

    def inverse(self):
        """Fr::inverse (src/fields/fr/u64/wrapper.rs:80-86) -> (Fr, status[n]); status 1 = None (zero input)."""
        return self._op("inverse")

    @staticmethod
    def from_le_bytes_mod_order(data, ctx=None):
        """Fr::from_le_bytes_mod_order for [n, 32], [n, 48] or [n, 64] byte strings (src/fields/fr.rs:82-94)."""
        c = ctx or default_context()
        width = int(data.shape[1])
        return Fr(c.fr_from_le_bytes_mod_order(data) if width == 32 else c.fr_from_wide_bytes(data), ctx)


class Encoding(_Bytes32):
    """Batch of `Encoding([u8; 32])` (src/ark_curve/encoding.rs:14-15)."""

    def vartime_decompress(self):
        """-> (Element, status[n]); status 1 = EncodingError::InvalidEncoding (encoding.rs:32-83)."""
        xyzt, st = self._ctx().decompress(self.data)
        return Element(xyzt, self.ctx), st

    def roundtrip(self):
        out, st = self._ctx().roundtrip(self.data)
        return Encoding(out, self.ctx), st

    def scalar_mul(self, scalars):
        """decompress(self) * scalars, compressed (src/min_curve/ops.rs:89-95)."""
        out, st = self._ctx().scalar_mul_var(self.data, scalars.data)
        return Encoding(out, self.ctx), st

    def unwrap_decompress(self):
        el, st = self.vartime_decompress()
        bad = st.cpu().numpy() if _is_torch(st) else st
        if bad.any():
            raise EncodingError("InvalidEncoding at index %d" % int(np.nonzero(bad)[0][0]))
        return el


class Element:
    """Batch of group elements in the reference's in-memory form: X, Y, Z, T as 4 Montgomery
    u64 limbs each (shape [n, 16]); src/min_curve/element.rs:31-38."""

    def __init__(self, xyzt, ctx=None):
        if not _is_torch(xyzt):
            xyzt = np.ascontiguousarray(np.asarray(xyzt, dtype=np.uint64)).reshape(-1, 16)
        self.data = xyzt
        self.ctx = ctx

    def _ctx(self):
        return self.ctx or default_context()

    def __len__(self):
        return int(self.data.shape[0])

    def __add__(self, other):
        """Element + Element (src/min_curve/element.rs:291-322)."""
        return Element(self._ctx().add(self.data, other.data), self.ctx)

    def __neg__(self):
        """-Element (src/min_curve/element.rs:324-332)."""
        return Element(self._ctx().neg(self.data), self.ctx)

    def is_identity(self):
        """Element::is_identity (src/min_curve/element.rs:113-117) -> u8[n]."""
        return self._ctx().is_identity(self.data)

    def double(self):
        """Element::double (src/min_curve/element.rs:119-136)."""
        return Element(self._ctx().double(self.data), self.ctx)

    def eq(self, other):
        """PartialEq for Element: x1*y2 == x2*y1 (src/min_curve/element.rs:334-340) -> u8[n]."""
        return self._ctx().eq(self.data, other.data)

    def vartime_compress(self):
        """Element::vartime_compress (src/ark_curve/encoding.rs:116-128)."""
        return Encoding(self._ctx().compress(self.data), self.ctx)

    def vartime_compress_to_field(self):
        """Element::vartime_compress_to_field (src/min_curve/element.rs:163-181) -> [n, 4] u64 Montgomery limbs."""
        return self._ctx().compress_to_field(self.data)

    def __mul__(self, scalars):
        """Element * Fr -> Element (src/min_curve/ops.rs:89-95)."""
        return Element(self._ctx().scalar_mul_var_element(self.data, scalars.data), self.ctx)

    @staticmethod
    def encode_to_curve_element(r):
        """Element::encode_to_curve (src/min_curve/element.rs:242-244) as an Element."""
        return Element(r._ctx().encode_to_curve_element(r.data), r.ctx)

    @staticmethod
    def hash_to_curve_element(r1, r2):
        """Element::hash_to_curve (src/min_curve/element.rs:235-240) as an Element."""
        return Element(r1._ctx().hash_to_curve_element(r1.data, r2.data), r1.ctx)

    @staticmethod
    def generator_mul_element(scalars):
        """Element::GENERATOR * scalars as Elements."""
        return Element(scalars._ctx().scalar_mul_base_element(scalars.data), scalars.ctx)

    @staticmethod
    def encode_to_curve(r):
        """Element::encode_to_curve (src/ark_curve/elligator.rs:74-76), returned compressed."""
        return Encoding(r._ctx().encode_to_curve(r.data), r.ctx)

    @staticmethod
    def hash_to_curve(r1, r2):
        """Element::hash_to_curve (src/ark_curve/elligator.rs:67-71), returned compressed."""
        return Encoding(r1._ctx().hash_to_curve(r1.data, r2.data), r1.ctx)

    @staticmethod
    def vartime_multiscalar_mul(scalars, points):
        """Element::vartime_multiscalar_mul(scalars, points) -> Encoding of the sum
        (src/ark_curve/element/projective.rs:99-117); `points` is an Element or Encoding batch."""
        enc, _, _ = points._ctx().msm(points.data, scalars.data)
        return Encoding(enc.reshape(1, 32) if not _is_torch(enc) else enc.reshape(1, 32), points.ctx)

    @staticmethod
    def generator_mul(scalars):
        """Element::GENERATOR * scalars, returned compressed."""
        return Encoding(scalars._ctx().scalar_mul_base(scalars.data), scalars.ctx)
