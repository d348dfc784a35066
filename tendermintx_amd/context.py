"""Context + array-level entry points over the C ABI."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import KIND_SKIP, KIND_STEP, Config, Report, check


def _indices(indices):
    """query indices (a sequence or a numpy array) as the contiguous uint64 host buffer the opening calls take"""
    if isinstance(indices, np.ndarray):
        return np.ascontiguousarray(indices.reshape(-1), dtype=np.uint64)
    return np.array([int(i) for i in indices], dtype=np.uint64)


class Context:
    """One tmx_ctx: a HIP stream, device scratch for `max_batch` proofs and the serializer programs for a fixed
    (VALIDATOR_SET_SIZE_MAX, chain id, SKIP_MAX) -- the const generics / TendermintConfig of the reference's
    SkipCircuit<N, CHAIN_ID_SIZE_BYTES, C> (reference circuits/skip.rs:104-111, circuits/config.rs:3-8)."""

    def __init__(self, n_max, chain_id=b"celestia", skip_max=100800, device=0, max_batch=1):
        self._L = _lib.lib()
        self.n_max, self.chain_id, self.skip_max, self.max_batch = int(n_max), bytes(chain_id), int(skip_max), int(max_batch)
        cfg = Config()
        cfg.n_max = self.n_max
        cfg.chain_id_len = len(self.chain_id)
        for i, b in enumerate(self.chain_id[:52]):
            cfg.chain_id[i] = b
        cfg.skip_max = self.skip_max
        cfg.device = device
        cfg.max_batch = self.max_batch
        h = C.c_void_p()
        st = self._L.tmx_ctx_create(C.byref(cfg), C.byref(h))
        self._h = h
        if st != 0:
            try:
                check(st, h if h else None)
            finally:
                if h:
                    self._L.tmx_ctx_destroy(h)
                    self._h = None

    def close(self):
        if getattr(self, "_h", None):
            self._L.tmx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def elem_count(self, kind):
        return int(self._L.tmx_elem_count(kind, self.n_max))

    def elem_stride(self, kind):
        return int(self._L.tmx_elem_stride(kind, self.n_max))

    def hint_elem_count(self, kind):
        return int(self._L.tmx_hint_elem_count(kind, self.n_max))

    # ---- host-buffer path
    def witness_batch(self, kind, proofs, targets, trusteds=None, want_elems=True, out=None):
        """proofs: bytes (n x 2336); targets: bytes (n x n_max x 256); trusteds: bytes (n x n_max x 48) for skip.
        out: optional preallocated np.uint64 array of n * elem_stride elements (e.g. a view of page-locked memory: the 1.1 GB of a
        256-proof batch come back at PCIe speed instead of through the runtime's pageable staging).
        Returns (np.uint64 [n, elem_count] or None, [report dict])."""
        n = len(proofs) // 2336
        assert len(proofs) == n * 2336 and len(targets) == n * self.n_max * 256
        if kind == KIND_SKIP:
            assert trusteds is not None and len(trusteds) == n * self.n_max * 48
        count, stride = self.elem_count(kind), self.elem_stride(kind)
        if want_elems and out is None:
            out = np.zeros(n * stride, dtype=np.uint64)
        elif want_elems:
            assert out.dtype == np.uint64 and out.size >= n * stride and out.flags["C_CONTIGUOUS"]
            out = out.reshape(-1)[:n * stride]
        else:
            out = None
        reps = (Report * n)()
        st = self._L.tmx_witness_batch(self._h, kind, n, bytes(proofs), bytes(targets), bytes(trusteds) if trusteds else None,
                                       out.ctypes.data if want_elems else None, out.size if want_elems else 0, reps)
        check(st, self._h)
        elems = out.reshape(n, stride)[:, :count] if want_elems else None
        return elems, [r.as_dict() for r in reps]

    def witness_batch_opts(self, kind, proofs, targets, trusteds=None, sections=_lib.SEC_ALL, fmt="u64", out=None):
        """tmx_witness_batch_opts: DENSE rows of the selected sections (_lib.SEC_HINT / SEC_DERIVED / SEC_ALL) as np.uint64 ("u64") or
        np.uint32 ("u32": every element of this witness is < 2^32).  Returns (array [n, row_elems], [report dict])."""
        n = len(proofs) // 2336
        assert len(proofs) == n * 2336 and len(targets) == n * self.n_max * 256
        if kind == KIND_SKIP:
            assert trusteds is not None and len(trusteds) == n * self.n_max * 48
        dt = np.uint32 if fmt == "u32" else np.uint64
        row = int(self._L.tmx_out_row_elems(kind, self.n_max, sections))
        if out is None:
            out = np.zeros(n * row, dtype=dt)
        else:
            assert out.flags["C_CONTIGUOUS"] and out.nbytes >= n * row * np.dtype(dt).itemsize
            out = out.reshape(-1).view(dt)[:n * row]
        reps = (Report * n)()
        st = self._L.tmx_witness_batch_opts(self._h, kind, n, bytes(proofs), bytes(targets), bytes(trusteds) if trusteds else None, sections,
                                            1 if fmt == "u32" else 0, out.ctypes.data, out.nbytes, reps)
        check(st, self._h)
        return out.reshape(n, row), [r.as_dict() for r in reps]

    def witness_batch_hint(self, kind, proofs, targets, trusteds=None, out=None, fmt="u32"):
        """Only the hint section H of every row (what the reference's hint writes to its output stream), narrowed to u32 by default."""
        return self.witness_batch_opts(kind, proofs, targets, trusteds, _lib.SEC_HINT, fmt, out)

    # ---- the typed value of the hint: SkipInputs<F> / StepInputs<F> field by field (include/tmx.h "TYPED VALUE")
    def value_layout(self, kind, sections=_lib.SEC_HINT):
        lay = _lib.ValueLayout()
        check(self._L.tmx_value_layout_of(kind, self.n_max, sections, C.byref(lay)), self._h)
        return lay

    def host_alloc(self, nbytes):
        """Page-locked host memory (tmx_host_alloc) as a np.uint8 array; release with host_free(array)."""
        p = self._L.tmx_host_alloc(self._h, nbytes)
        if not p:
            raise MemoryError(f"tmx_host_alloc({nbytes})")
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p
        return a

    def host_free(self, a):
        p = getattr(self, "_pinned", {}).pop(a.ctypes.data, None)
        if p:
            self._L.tmx_host_free(self._h, p)

    def inputs_value_batch(self, kind, proofs, targets, trusteds=None, sections=_lib.SEC_HINT, out=None):
        """tmx_inputs_value_batch: n proofs -> np.uint8 [n, layout.bytes] (one typed value per row) + the layout.  proofs / targets /
        trusteds: bytes, or np.uint8 arrays (e.g. views of host_alloc memory: nothing is copied on the way in)."""
        ptr = lambda b: b.ctypes.data if isinstance(b, np.ndarray) else bytes(b)
        size = lambda b: b.nbytes if isinstance(b, np.ndarray) else len(b)
        n = size(proofs) // 2336
        assert size(proofs) == n * 2336 and size(targets) == n * self.n_max * 256
        if kind == KIND_SKIP:
            assert trusteds is not None and size(trusteds) == n * self.n_max * 48
        lay = self.value_layout(kind, sections)
        if out is None:
            out = np.zeros(n * lay.bytes, dtype=np.uint8)
        else:
            assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size >= n * lay.bytes
            out = out.reshape(-1)[:n * lay.bytes]
        st = self._L.tmx_inputs_value_batch(self._h, kind, n, ptr(proofs), ptr(targets), ptr(trusteds) if trusteds is not None else None, sections,
                                            out.ctypes.data, out.nbytes)
        check(st, self._h)
        return out.reshape(n, lay.bytes), lay

    def inputs_value_batch_device(self, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out, sections=_lib.SEC_HINT, stream=None):
        check(self._L.tmx_inputs_value_batch_device(self._h, kind, n_proofs, d_proofs, d_targets, d_trusteds, sections, d_out, self._stream(stream)), self._h)

    def witness_batch_device_sections(self, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out, d_reports, sections, stream=None):
        check(self._L.tmx_witness_batch_device_sections(self._h, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out, d_reports,
                                                        self._stream(stream), sections), self._h)

    def trace_elem_count(self, kind):
        return int(self._L.tmx_trace_elem_count(kind, self.n_max))

    def trace_rows_device(self, kind, n_proofs, d_targets, d_trusteds, d_trace_out, sections=_lib.TRACE_ALL, stream=None):
        """Level-2 trace rows of the batch whose Level-1 witness this context computed last (same stream): tmx_trace_rows_device."""
        check(self._L.tmx_trace_rows_device(self._h, kind, n_proofs, d_targets, d_trusteds, d_trace_out, sections, self._stream(stream)), self._h)

    def valid_skip_batch(self, start, n_start, targets, n_targets, sigs, n_sigs):
        """is_valid_skip for len(n_targets) candidates.  start: bytes [n_max x 32]; targets, sigs: bytes [n_cand x n_max x 32].
        Returns (valid [bool], shared power [int], total power [int])."""
        nc = len(n_targets)
        assert len(targets) == nc * self.n_max * 32 == len(sigs)
        nt, ns = (C.c_uint32 * nc)(*n_targets), (C.c_uint32 * nc)(*n_sigs)
        valid, sh, to = (C.c_uint8 * nc)(), (C.c_uint64 * nc)(), (C.c_uint64 * nc)()
        check(self._L.tmx_valid_skip_batch(self._h, nc, bytes(start), n_start, bytes(targets), nt, bytes(sigs), ns, valid, sh, to), self._h)
        return [bool(v) for v in valid], list(sh), list(to)

    def eddsa_lanes(self, lanes):
        n = len(lanes) // 256
        out = np.zeros(n * _lib.ED_STRIDE, dtype=np.uint8)
        check(self._L.tmx_eddsa_lanes(self._h, n, bytes(lanes), out.ctypes.data), self._h)
        return out.reshape(n, _lib.ED_STRIDE)

    # ---- device-resident path (raw device pointers, e.g. torch tensors' data_ptr())
    def _stream(self, stream):
        """stream=None -> the context's own stream; an int (e.g. torch.cuda.current_stream().cuda_stream, 0 = the HIP default
        stream) is used exactly as given."""
        return self._L.tmx_ctx_stream(self._h) if stream is None else (stream or None)

    def witness_batch_device(self, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out, d_reports, stream=None):
        check(self._L.tmx_witness_batch_device(self._h, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out, d_reports,
                                               self._stream(stream)), self._h)

    def selftest_fe_invert(self, values):
        """values: ints; returns [(fermat_inverse, safegcd_inverse)] mod 2^255 - 19 as computed on the GPU (self-test hook)."""
        n = len(values)
        inp = np.zeros((n, 8), dtype=np.uint32)
        for i, v in enumerate(values):
            for k in range(8):
                inp[i, k] = (int(v) >> (32 * k)) & 0xFFFFFFFF
        out = np.zeros((n, 16), dtype=np.uint32)
        check(self._L.tmx_selftest_fe_invert(self._h, n, inp.ctypes.data, out.ctypes.data), self._h)
        conv = lambda w: sum(int(w[k]) << (32 * k) for k in range(8))
        return [(conv(out[i, :8]), conv(out[i, 8:])) for i in range(n)]

    def selftest_f16(self, words, doublings):
        """words: uint32 array (n, 128); returns uint32 (n, 256) -- see tmx_selftest_f16 (self-test hook)."""
        inp = np.ascontiguousarray(words, dtype=np.uint32)
        n = inp.shape[0]
        out = np.zeros((n, 256), dtype=np.uint32)
        check(self._L.tmx_selftest_f16(self._h, n, doublings, inp.ctypes.data, out.ctypes.data), self._h)
        return out

    # ---- Goldilocks NTT / coset LDE (device pointers; columns of 2**log_n u64, column c at element c << log_n)
    def ntt_set_domain(self, root_2_32, coset_shift):
        """Domain constants of the NTT / LDE: a primitive 2^32-th root of unity and the coset shift (default: plonky2's, as recalled)."""
        check(self._L.tmx_ntt_set_domain(self._h, C.c_uint64(root_2_32), C.c_uint64(coset_shift)), self._h)

    def ntt_device(self, log_n, n_cols, d_in, d_out, inverse=False, stream=None):
        check(self._L.tmx_ntt_goldilocks_device(self._h, log_n, n_cols, d_in, d_out, 1 if inverse else 0, self._stream(stream)), self._h)

    def lde_device(self, log_n, log_blowup, n_cols, d_in, d_out, stream=None):
        check(self._L.tmx_lde_goldilocks_device(self._h, log_n, log_blowup, n_cols, d_in, d_out, self._stream(stream)), self._h)

    # ---- Poseidon over Goldilocks + Merkle caps (tmx_poseidon_*)
    def poseidon_set_constants(self, round_constants=None, mds_circ=None, mds_diag=None):
        arr = lambda v, n: (C.c_uint64 * n)(*[int(x) for x in v]) if v is not None else None
        check(self._L.tmx_poseidon_set_constants(self._h, arr(round_constants, 360), arr(mds_circ, 12), arr(mds_diag, 12)), self._h)

    def poseidon_permute(self, states):
        a = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 12)
        out = np.zeros_like(a)
        check(self._L.tmx_poseidon_permute(self._h, a.shape[0], a.ctypes.data, out.ctypes.data), self._h)
        return out

    def poseidon_merkle_digests(self, log_n, cap_height):
        return int(self._L.tmx_poseidon_merkle_digests(log_n, cap_height))

    def poseidon_merkle_device(self, log_n, n_cols, d_cols, cap_height, d_levels, stream=None):
        check(self._L.tmx_poseidon_merkle_device(self._h, log_n, n_cols, d_cols, cap_height, d_levels, self._stream(stream)), self._h)

    # ---- openings of a Poseidon Merkle tree (rows + paths) and their verification; indices: a sequence or numpy array, host side
    def poseidon_merkle_path_len(self, log_n, cap_height):
        return int(self._L.tmx_poseidon_merkle_path_len(log_n, cap_height))

    def poseidon_merkle_open_device(self, log_n, n_cols, d_cols, cap_height, d_levels, indices, d_rows, d_paths, stream=None):
        """d_rows: [n_queries][n_cols] u64, d_paths: [n_queries][path_len][4] u64 (device pointers)"""
        idx = _indices(indices)
        check(self._L.tmx_poseidon_merkle_open_device(self._h, log_n, n_cols, d_cols, cap_height, d_levels, idx.size, idx.ctypes.data, d_rows, d_paths,
                                                      self._stream(stream)), self._h)

    def poseidon_merkle_verify_device(self, log_n, n_cols, cap_height, d_cap, indices, d_rows, d_paths, d_ok, stream=None):
        """d_ok: [n_queries] u32, 1 where the opening leads to the cap"""
        idx = _indices(indices)
        check(self._L.tmx_poseidon_merkle_verify_device(self._h, log_n, n_cols, cap_height, d_cap, idx.size, idx.ctypes.data, d_rows, d_paths, d_ok,
                                                        self._stream(stream)), self._h)

    def eddsa_lanes_device(self, n_lanes, d_lanes, d_ed_out, stream=None):
        check(self._L.tmx_eddsa_lanes_device(self._h, n_lanes, d_lanes, d_ed_out, self._stream(stream)), self._h)

    def finish_batch_device(self, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_ed, d_out, d_reports, stream=None):
        check(self._L.tmx_finish_batch_device(self._h, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_ed, d_out, d_reports, self._stream(stream)),
              self._h)

    # ---- the commit pipeline on the device: section rows -> columns -> LDE -> Poseidon Merkle cap
    def trace_commit_shape(self, kind, section):
        lg, w = C.c_uint32(), C.c_uint32()
        check(self._L.tmx_trace_commit_shape(kind, self.n_max, section, C.byref(lg), C.byref(w)), self._h)
        return lg.value, w.value

    def trace_commit_device(self, kind, n_proofs, section, log_blowup, cap_height, d_trace_rows, d_cap, stream=None):
        check(self._L.tmx_trace_commit_device(self._h, kind, n_proofs, section, log_blowup, cap_height, d_trace_rows, d_cap, self._stream(stream)), self._h)

    def trace_commit_last_ms(self):
        ms = (C.c_float * 3)()
        check(self._L.tmx_trace_commit_last_ms(self._h, ms), self._h)
        return {"columns": ms[0], "lde": ms[1], "merkle": ms[2]}

    def trace_commit_last_shape(self):
        """(log_rows + log_blowup, n_proofs * width, cap_height) of the context's most recent commit; TmxError if there is none to open"""
        lg, nc, ch = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(self._L.tmx_trace_commit_last_shape(self._h, C.byref(lg), C.byref(nc), C.byref(ch)), self._h)
        return lg.value, nc.value, ch.value

    def trace_commit_open_device(self, indices, d_rows, d_paths, stream=None):
        """openings of the most recent trace_commit_device (same stream, after it): rows [n_queries][n_cols], paths [n_queries][path_len][4]"""
        idx = _indices(indices)
        check(self._L.tmx_trace_commit_open_device(self._h, idx.size, idx.ctypes.data, d_rows, d_paths, self._stream(stream)), self._h)

    # ---- a batched FRI low-degree proof over committed columns (include/tmx.h "a batched FRI low-degree proof"); params: a dict or
    # _lib.FriParams with log_n, n_cols, cap_height, log_blowup, arity_bits, final_log_max, n_queries
    @staticmethod
    def _fri_params(params):
        if isinstance(params, _lib.FriParams):
            return params
        return _lib.FriParams(**{k: int(v) for k, v in params.items()})

    def fri_layout(self, params):
        """the schedule and every u64 offset of the proof (host only): a dict; TmxError on parameters the ABI refuses"""
        return fri_layout(params, self._L)

    def fri_prove_device(self, params, d_cols, d_levels, d_proof, stream=None):
        """a proof over caller columns (d_cols, d_levels: what lde_goldilocks_device / poseidon_merkle_device wrote) into d_proof[words]"""
        check(self._L.tmx_fri_prove_device(self._h, C.byref(self._fri_params(params)), d_cols, d_levels, d_proof, self._stream(stream)), self._h)

    def trace_commit_fri_device(self, params, d_proof, stream=None):
        """a proof over the most recent trace_commit_device (same stream, after it); the parameters must match that commit"""
        check(self._L.tmx_trace_commit_fri_device(self._h, C.byref(self._fri_params(params)), d_proof, self._stream(stream)), self._h)

    def fri_verify_device(self, params, d_cap, d_proof, d_ok, stream=None):
        """d_ok[n_queries] u32: 1 where the query checks against the commit cap d_cap"""
        check(self._L.tmx_fri_verify_device(self._h, C.byref(self._fri_params(params)), d_cap, d_proof, d_ok, self._stream(stream)), self._h)

    def fri_last_degree_ok(self):
        """(blocks) True if the last prove's dropped final coefficients were all zero"""
        st = self._L.tmx_fri_last_degree_ok(self._h)
        if st < 0:
            check(st, self._h)
        return st == 1

    def fri_last_ms(self):
        ms = (C.c_float * 4)()
        check(self._L.tmx_fri_last_ms(self._h, ms), self._h)
        return {"combine": ms[0], "layers": ms[1], "final": ms[2], "openings": ms[3]}

    # ---- out-of-domain openings (DEEP-FRI; include/tmx.h "out-of-domain openings"): the same params as the FRI calls; a proof is
    # deep_proof_words(params) words: the openings section, then the FRI part
    def deep_prove_device(self, params, d_cols, d_levels, d_proof, stream=None):
        """a DEEP proof over caller columns (extended, with their tree) into d_proof"""
        check(self._L.tmx_deep_prove_device(self._h, C.byref(self._fri_params(params)), d_cols, d_levels, d_proof, self._stream(stream)), self._h)

    def trace_commit_deep_device(self, params, d_proof, stream=None):
        """a DEEP proof over the most recent trace_commit_device (same stream, after it); the parameters must match that commit"""
        check(self._L.tmx_trace_commit_deep_device(self._h, C.byref(self._fri_params(params)), d_proof, self._stream(stream)), self._h)

    def deep_verify_device(self, params, d_cap, d_proof, d_ok, stream=None):
        """d_ok[n_queries] u32: 1 where the query of the DEEP proof checks against the commit cap d_cap"""
        check(self._L.tmx_deep_verify_device(self._h, C.byref(self._fri_params(params)), d_cap, d_proof, d_ok, self._stream(stream)), self._h)

    def deep_last_zeta(self):
        """(blocks) zeta of the last DEEP prove as (c0, c1); TmxError if the last prove was a plain FRI prove or there was none"""
        z = (C.c_uint64 * 2)()
        check(self._L.tmx_deep_last_zeta(self._h, z), self._h)
        return int(z[0]), int(z[1])

    # ---- proof of work (include/tmx.h "proof of work"): the grinding variants of both proofs; params: the FRI params, pow_bits (1 .. 24)
    # and deep (False: the FRI proof, True: the DEEP proof); a proof is pow_proof_words(params, pow_bits, deep) words, the nonce last
    @staticmethod
    def _pow_params(params, pow_bits, deep):
        return _lib.PowParams(fri=Context._fri_params(params), pow_bits=int(pow_bits), deep=int(deep))

    def pow_proof_words(self, params, pow_bits, deep=False):
        return pow_proof_words(params, pow_bits, deep, self._L)

    def pow_prove_device(self, params, pow_bits, deep, d_cols, d_levels, d_proof, stream=None):
        """a grinding proof over caller columns (as fri_prove_device / deep_prove_device) into d_proof"""
        check(self._L.tmx_pow_prove_device(self._h, C.byref(self._pow_params(params, pow_bits, deep)), d_cols, d_levels, d_proof,
                                           self._stream(stream)), self._h)

    def trace_commit_pow_device(self, params, pow_bits, deep, d_proof, stream=None):
        """a grinding proof over the most recent trace_commit_device (same stream, after it); the parameters must match that commit"""
        check(self._L.tmx_trace_commit_pow_device(self._h, C.byref(self._pow_params(params, pow_bits, deep)), d_proof, self._stream(stream)), self._h)

    def pow_verify_device(self, params, pow_bits, deep, d_cap, d_proof, d_ok, stream=None):
        """d_ok[n_queries] u32: 1 where the query of the grinding proof checks against the commit cap d_cap"""
        check(self._L.tmx_pow_verify_device(self._h, C.byref(self._pow_params(params, pow_bits, deep)), d_cap, d_proof, d_ok,
                                            self._stream(stream)), self._h)

    def pow_last(self):
        """(blocks) (nonce, candidates evaluated) of the last grinding prove; TmxError if the last prove was not one, or (status -4) if
        its search gave up"""
        nonce, tried = C.c_uint64(), C.c_uint64()
        check(self._L.tmx_pow_last(self._h, C.byref(nonce), C.byref(tried)), self._h)
        return int(nonce.value), int(tried.value)

    # ---- one DEEP-FRI proof over several oracles of different sizes, and the commit set (include/tmx.h "one DEEP-FRI proof over several
    # oracles"); params: a dict with log_blowup, cap_height, arity_bits, final_log_max, n_queries, pow_bits (0: no grinding) and the oracle
    # list log_n, n_cols (sequences of equal length, by non-increasing log_n), or a _lib.BatchParams
    @staticmethod
    def _batch_params(params):
        if isinstance(params, _lib.BatchParams):
            return params
        p = dict(params)
        log_n, n_cols = [int(x) for x in p.pop("log_n")], [int(x) for x in p.pop("n_cols")]
        n = int(p.pop("n_oracles", len(log_n)))
        if len(log_n) != len(n_cols) or len(log_n) > _lib.BATCH_MAX_ORACLES:
            raise _lib.TmxError(-1, "log_n and n_cols must have the same length, at most 8")
        return _lib.BatchParams(n_oracles=n, log_n=(C.c_uint32 * _lib.BATCH_MAX_ORACLES)(*log_n),
                                n_cols=(C.c_uint32 * _lib.BATCH_MAX_ORACLES)(*n_cols), **{k: int(v) for k, v in p.items()})

    def batch_layout(self, params):
        return batch_layout(params, self._L)

    def batch_prove_device(self, params, d_cols, d_levels, d_proof, stream=None):
        """one proof over caller oracles: d_cols[k], d_levels[k] device pointers of oracle k's extended columns and tree"""
        p = self._batch_params(params)
        cols, levels = (C.c_void_p * p.n_oracles)(*d_cols), (C.c_void_p * p.n_oracles)(*d_levels)
        check(self._L.tmx_batch_prove_device(self._h, C.byref(p), cols, levels, d_proof, self._stream(stream)), self._h)

    def batch_verify_device(self, params, d_caps, d_proof, d_ok, stream=None):
        """d_ok[n_queries] u32: 1 where the query checks against the K caps concatenated at d_caps"""
        check(self._L.tmx_batch_verify_device(self._h, C.byref(self._batch_params(params)), d_caps, d_proof, d_ok, self._stream(stream)), self._h)

    def trace_commit_set_device(self, kind, n_proofs, sections, log_blowup, cap_height, d_trace_rows, d_caps, stream=None):
        """commits every row table of the mask `sections` side by side; d_caps receives the caps in the set's oracle order"""
        check(self._L.tmx_trace_commit_set_device(self._h, kind, n_proofs, sections, log_blowup, cap_height, d_trace_rows, d_caps,
                                                  self._stream(stream)), self._h)

    def trace_commit_set_streamed_device(self, kind, n_proofs, sections, streamed, chunk_cols, log_blowup, cap_height, d_trace_rows, d_caps,
                                         stream=None):
        """trace_commit_set_device with the members of the mask `streamed` kept as pre-LDE columns + tree levels only and extended
        chunk_cols columns (a multiple of 8) at a time; caps, shape and proofs are the resident set's word for word"""
        check(self._L.tmx_trace_commit_set_streamed_device(self._h, kind, n_proofs, sections, streamed, chunk_cols, log_blowup, cap_height,
                                                           d_trace_rows, d_caps, self._stream(stream)), self._h)

    def trace_commit_set_bytes(self, kind, n_proofs, sections, streamed, chunk_cols, log_blowup, cap_height):
        """(host only) the bytes trace_commit_set_streamed_device checks against free memory: set scratch + the LDE's scratch; 0 for
        arguments it would refuse"""
        return trace_commit_set_bytes(kind, self.n_max, n_proofs, sections, streamed, chunk_cols, log_blowup, cap_height, self._L)

    def trace_commit_set_shape(self):
        """(params dict with the set's n_oracles, log_blowup, cap_height, log_n, n_cols and the other fields zero, [section bit per oracle])"""
        p, sec = _lib.BatchParams(), (C.c_uint32 * _lib.BATCH_MAX_ORACLES)()
        check(self._L.tmx_trace_commit_set_shape(self._h, C.byref(p), sec), self._h)
        K = p.n_oracles
        return (dict(log_blowup=p.log_blowup, cap_height=p.cap_height, arity_bits=0, final_log_max=0, n_queries=0, pow_bits=0,
                     log_n=list(p.log_n[:K]), n_cols=list(p.n_cols[:K])), list(sec[:K]))

    def trace_commit_set_prove_device(self, params, d_proof, stream=None):
        """one proof over the commit set (same stream, after it); the oracle list, log_blowup and cap_height must match the set"""
        check(self._L.tmx_trace_commit_set_prove_device(self._h, C.byref(self._batch_params(params)), d_proof, self._stream(stream)), self._h)

    # ---- the constraint quotient of the ladder rows (include/tmx.h "the constraint quotient of the ladder rows")
    def air_ladder_quotient_device(self, log_n, log_blowup, cap_height, n_proofs, d_cols, d_cap, d_quot, stream=None, proof_range=None,
                                   accumulate=False):
        """gamma from the trace cap d_cap, then the constraint quotient of the n_proofs * 65 extended ladder columns at d_cols into d_quot
        (planar, 2 << log_n words).  proof_range = (lo, hi): those proofs' terms only, added to what d_quot holds if accumulate"""
        if proof_range is None and not accumulate:
            check(self._L.tmx_air_ladder_quotient_device(self._h, log_n, log_blowup, cap_height, n_proofs, d_cols, d_cap, d_quot,
                                                         self._stream(stream)), self._h)
            return
        lo, hi = proof_range if proof_range is not None else (0, n_proofs)
        check(self._L.tmx_air_ladder_quotient_range_device(self._h, log_n, log_blowup, cap_height, n_proofs, lo, hi, int(accumulate), d_cols, d_cap,
                                                           d_quot, self._stream(stream)), self._h)

    def air_last_gamma(self):
        """(blocks) gamma of the last quotient call as (c0, c1); TmxError if there was none"""
        g = (C.c_uint64 * 2)()
        check(self._L.tmx_air_last_gamma(self._h, g), self._h)
        return int(g[0]), int(g[1])

    def air_verify_device(self, params, k_trace, d_caps, d_proof, d_ok, stream=None):
        """batch_verify_device, then the constraint identity at zeta for oracle k_trace (the ladders) and k_trace + 1 (its quotient): a
        failed identity clears every d_ok[q]"""
        check(self._L.tmx_air_verify_device(self._h, C.byref(self._batch_params(params)), k_trace, d_caps, d_proof, d_ok, self._stream(stream)),
              self._h)

    def trace_commit_set_air_device(self, d_cap_q, stream=None):
        """adds the ladders' constraint quotient to the commit set as the oracle right after the ladders; d_cap_q receives its cap"""
        check(self._L.tmx_trace_commit_set_air_device(self._h, d_cap_q, self._stream(stream)), self._h)

    # ---- constraint set 2: the boundary constraints of the ladder rows (include/tmx.h)
    def air_ladder_public_shape(self, kind, n_proofs):
        """(log2 K, columns) of the public table of n_proofs proofs at this context's n_max"""
        return air_ladder_public_shape(kind, self.n_max, n_proofs)

    def air_ladder_public_device(self, kind, n_proofs, d_elems, d_pub, stream=None):
        """the public table (column-major, 17 n_proofs columns of K words at d_pub) from the element rows witness_batch_device wrote"""
        check(self._L.tmx_air_ladder_public_device(self._h, kind, n_proofs, d_elems, d_pub, self._stream(stream)), self._h)

    def air_ladder_boundary_quotient_device(self, log_n, log_blowup, cap_height, n_proofs, d_cols, d_cap, d_pub, d_quot, stream=None,
                                            proof_range=None, accumulate=False):
        """air_ladder_quotient_device for constraint set 2: the 33 row constraints and the 32 boundary constraints against d_pub"""
        if proof_range is None and not accumulate:
            check(self._L.tmx_air_ladder_boundary_quotient_device(self._h, log_n, log_blowup, cap_height, n_proofs, d_cols, d_cap, d_pub, d_quot,
                                                                  self._stream(stream)), self._h)
            return
        lo, hi = proof_range if proof_range is not None else (0, n_proofs)
        check(self._L.tmx_air_ladder_boundary_quotient_range_device(self._h, log_n, log_blowup, cap_height, n_proofs, lo, hi, int(accumulate), d_cols,
                                                                    d_cap, d_pub, d_quot, self._stream(stream)), self._h)

    def air_boundary_verify_device(self, params, k_trace, d_caps, d_proof, d_pub, d_ok, stream=None):
        """batch_verify_device, then the set-2 identity at zeta against the public table d_pub: a failed identity clears every d_ok[q]"""
        check(self._L.tmx_air_boundary_verify_device(self._h, C.byref(self._batch_params(params)), k_trace, d_caps, d_proof, d_pub, d_ok,
                                                     self._stream(stream)), self._h)

    def trace_commit_set_air_boundary_device(self, d_pub, d_cap_q, stream=None):
        """trace_commit_set_air_device for constraint set 2; the two exclude each other on one set"""
        check(self._L.tmx_trace_commit_set_air_boundary_device(self._h, d_pub, d_cap_q, self._stream(stream)), self._h)

    # ---- constraint set 3: the round constraints of the SHA-256 tables (include/tmx.h)
    def air_sha256_helper_device(self, log_rows, n_proofs, d_table, d_helper, stream=None):
        """the helper oracle (300 n_proofs columns of 2^log_rows words at d_helper) from the pre-LDE table columns (9 n_proofs) at d_table"""
        check(self._L.tmx_air_sha256_helper_device(self._h, log_rows, n_proofs, d_table, d_helper, self._stream(stream)), self._h)

    def air_sha256_quotient_device(self, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper, d_quot, stream=None,
                                   proof_range=None, accumulate=0):
        """gamma from the table cap and the helper cap, then the quotient of the 315 constraints per proof over the extended table and helper
        columns into d_quot (planar, 2 << log_n words).  proof_range = (lo, hi): those proofs' terms only, d_cols still the whole table's
        column 0 but d_helper_cols the first helper column of proof lo (a buffer that holds the piece alone will do); added to what d_quot
        holds if accumulate"""
        if proof_range is not None or accumulate:
            lo, hi = proof_range if proof_range is not None else (0, n_proofs)
            check(self._L.tmx_air_sha256_quotient_range_device(self._h, log_n, log_blowup, cap_height, n_proofs, lo, hi, int(accumulate), d_cols,
                                                               d_helper_cols, d_cap, d_cap_helper, d_quot, self._stream(stream)), self._h)
            return
        check(self._L.tmx_air_sha256_quotient_device(self._h, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper,
                                                     d_quot, self._stream(stream)), self._h)

    def air_sha256_verify_device(self, params, k_trace, d_caps, d_proof, d_ok, stream=None):
        """batch_verify_device, then the set-3 identity at zeta for the oracles k_trace (table), k_trace + 1 (helper), k_trace + 2 (quotient)"""
        check(self._L.tmx_air_sha256_verify_device(self._h, C.byref(self._batch_params(params)), k_trace, d_caps, d_proof, d_ok,
                                                   self._stream(stream)), self._h)

    def trace_commit_set_air_sha256_device(self, section, d_cap_h, d_cap_q, stream=None):
        """adds the helper and the quotient of the resident member `section` (SHA256, TREE or HEADER) to the commit set, directly behind it"""
        check(self._L.tmx_trace_commit_set_air_sha256_device(self._h, section, d_cap_h, d_cap_q, self._stream(stream)), self._h)

    # ---- constraint set 4: the message schedule of the SHA-256 tables (include/tmx.h)
    def air_sha256_sched_helper_device(self, log_rows, n_proofs, d_table, d_helper, stream=None):
        """the schedule helper (115 n_proofs columns of 2^log_rows words at d_helper) from the pre-LDE table columns (9 n_proofs) at d_table"""
        check(self._L.tmx_air_sha256_sched_helper_device(self._h, log_rows, n_proofs, d_table, d_helper, self._stream(stream)), self._h)

    def air_sha256_sched_quotient_device(self, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper, d_quot,
                                         stream=None, proof_range=None, accumulate=0):
        """gamma from the table cap and the helper cap, then the quotient of the 117 constraints per proof over the extended table and helper
        columns into d_quot (planar, 2 << log_n words); proof_range and accumulate as in air_sha256_quotient_device"""
        if proof_range is not None or accumulate:
            lo, hi = proof_range if proof_range is not None else (0, n_proofs)
            check(self._L.tmx_air_sha256_sched_quotient_range_device(self._h, log_n, log_blowup, cap_height, n_proofs, lo, hi, int(accumulate), d_cols,
                                                                     d_helper_cols, d_cap, d_cap_helper, d_quot, self._stream(stream)), self._h)
            return
        check(self._L.tmx_air_sha256_sched_quotient_device(self._h, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap,
                                                           d_cap_helper, d_quot, self._stream(stream)), self._h)

    def air_sha256_sched_verify_device(self, params, k_trace, k_helper, d_caps, d_proof, d_ok, stream=None):
        """batch_verify_device, then the set-4 identity at zeta for the oracles k_trace (table), k_helper (helper), k_helper + 1 (quotient)"""
        check(self._L.tmx_air_sha256_sched_verify_device(self._h, C.byref(self._batch_params(params)), k_trace, k_helper, d_caps, d_proof, d_ok,
                                                         self._stream(stream)), self._h)

    def trace_commit_set_air_sha256_sched_device(self, section, d_cap_h, d_cap_q, stream=None):
        """adds the schedule helper and quotient of the resident member `section` (SHA256, TREE or HEADER) to the commit set, behind the
        table or behind set 3's pair"""
        check(self._L.tmx_trace_commit_set_air_sha256_sched_device(self._h, section, d_cap_h, d_cap_q, self._stream(stream)), self._h)

    # ---- constraint set 5: the block starts of the SHA-256 tables (include/tmx.h)
    def air_sha256_init_helper_device(self, log_rows, n_proofs, chain, d_table, d_helper, stream=None):
        """the block-start helper (315 n_proofs columns of 2^log_rows words at d_helper) from the pre-LDE table columns (9 n_proofs) at
        d_table; chain = 0: every block a hash of its own (T.3), chain = 1: pairs of blocks on 128-row boundaries (T.5, T.6)"""
        check(self._L.tmx_air_sha256_init_helper_device(self._h, log_rows, n_proofs, chain, d_table, d_helper, self._stream(stream)), self._h)

    def air_sha256_init_quotient_device(self, log_n, log_blowup, cap_height, n_proofs, chain, d_cols, d_helper_cols, d_cap, d_cap_helper, d_quot,
                                        stream=None, proof_range=None, accumulate=0):
        """gamma from the table cap and the helper cap, then the quotient of the 337 constraints per proof over the extended table and helper
        columns into d_quot (planar, 2 << log_n words); proof_range and accumulate as in air_sha256_quotient_device"""
        if proof_range is not None or accumulate:
            lo, hi = proof_range if proof_range is not None else (0, n_proofs)
            check(self._L.tmx_air_sha256_init_quotient_range_device(self._h, log_n, log_blowup, cap_height, n_proofs, chain, lo, hi, int(accumulate),
                                                                    d_cols, d_helper_cols, d_cap, d_cap_helper, d_quot, self._stream(stream)),
                  self._h)
            return
        check(self._L.tmx_air_sha256_init_quotient_device(self._h, log_n, log_blowup, cap_height, n_proofs, chain, d_cols, d_helper_cols, d_cap,
                                                          d_cap_helper, d_quot, self._stream(stream)), self._h)

    def air_sha256_init_verify_device(self, params, k_trace, k_helper, chain, d_caps, d_proof, d_ok, stream=None):
        """batch_verify_device, then the set-5 identity at zeta for the oracles k_trace (table), k_helper (helper), k_helper + 1 (quotient)"""
        check(self._L.tmx_air_sha256_init_verify_device(self._h, C.byref(self._batch_params(params)), k_trace, k_helper, chain, d_caps, d_proof,
                                                        d_ok, self._stream(stream)), self._h)

    def trace_commit_set_air_sha256_init_device(self, section, d_cap_h, d_cap_q, stream=None):
        """adds the block-start helper and quotient of the resident member `section` (SHA256, TREE or HEADER) to the commit set, behind the
        last helper/quotient pair that already follows the table"""
        check(self._L.tmx_trace_commit_set_air_sha256_init_device(self._h, section, d_cap_h, d_cap_q, self._stream(stream)), self._h)

    # ---- constraint set 6: the SHA-256 tables' link to Level-1 (include/tmx.h): the public table and the helper
    def air_sha256_public_shape(self, kind, section, n_proofs):
        """(log2 K, columns) of the public table of `section` (SHA256, TREE or HEADER) of n_proofs proofs at this context's n_max"""
        return air_sha256_public_shape(kind, section, self.n_max, n_proofs)

    def air_sha256_public_device(self, kind, section, n_proofs, d_elems, d_pub, stream=None):
        """the public table of `section` (column-major, 26 n_proofs columns of K words at d_pub: per block the sixteen message words, the
        digest, new, chn) from the element rows witness_batch_device wrote"""
        check(self._L.tmx_air_sha256_public_device(self._h, kind, section, n_proofs, d_elems, d_pub, self._stream(stream)), self._h)

    def air_sha256_link_helper_device(self, log_rows, n_proofs, d_table, d_pub, d_helper, stream=None):
        """the link helper (33 n_proofs columns of 2^log_rows words at d_helper) from the pre-LDE table columns (9 n_proofs) at d_table and
        the flags of the public table (26 n_proofs columns of 2^(log_rows - 6) words) at d_pub"""
        check(self._L.tmx_air_sha256_link_helper_device(self._h, log_rows, n_proofs, d_table, d_pub, d_helper, self._stream(stream)), self._h)

    # ---- constraint set 10: the SHA-512 table's link to Level-1 (include/tmx.h): the public table and the helper
    def air_sha512_public_shape(self, kind, n_proofs):
        """(log2 K, columns) of the public table of T.2 of n_proofs proofs at this context's n_max"""
        return air_sha512_public_shape(kind, self.n_max, n_proofs)

    def air_sha512_public_device(self, kind, n_proofs, d_elems, d_pub, stream=None):
        """the public table of T.2 (column-major, 49 n_proofs columns of K words at d_pub: per block slot the sixteen message words and the
        digest in low / high limbs, lv) from the element rows witness_batch_device wrote"""
        check(self._L.tmx_air_sha512_public_device(self._h, kind, n_proofs, d_elems, d_pub, self._stream(stream)), self._h)

    def air_sha512_link_helper_device(self, log_rows, n_proofs, d_table, d_pub, d_helper, stream=None):
        """the link helper (65 n_proofs columns of 2^log_rows words at d_helper) from the pre-LDE table columns (18 n_proofs) at d_table and
        lv of the public table (49 n_proofs columns, one row per 80-row block slot, padded to a power of two) at d_pub"""
        check(self._L.tmx_air_sha512_link_helper_device(self._h, log_rows, n_proofs, d_table, d_pub, d_helper, self._stream(stream)), self._h)

    def air_sha512_link_quotient_device(self, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper, d_pub, d_quot,
                                        stream=None, proof_range=None, accumulate=0):
        """the five planes filled and extended, gamma from the table cap, the helper cap and the digest of d_pub, then the quotient of the 115
        constraints per proof over the extended table and helper columns into d_quot (planar, 2 << log_n words); proof_range and accumulate
        as in air_sha256_quotient_device: the piece that starts at proof 0 carries the public polynomial"""
        if proof_range is not None or accumulate:
            lo, hi = proof_range if proof_range is not None else (0, n_proofs)
            check(self._L.tmx_air_sha512_link_quotient_range_device(self._h, log_n, log_blowup, cap_height, n_proofs, lo, hi, int(accumulate), d_cols,
                                                                    d_helper_cols, d_cap, d_cap_helper, d_pub, d_quot, self._stream(stream)), self._h)
            return
        check(self._L.tmx_air_sha512_link_quotient_device(self._h, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper,
                                                          d_pub, d_quot, self._stream(stream)), self._h)

    def air_sha512_link_verify_device(self, params, k_trace, k_helper, d_caps, d_proof, d_pub, d_ok, stream=None):
        """batch_verify_device, then the set-10 identity at zeta for the oracles k_trace (table), k_helper (helper), k_helper + 1 (quotient)
        against the public table at d_pub, which the verifier hashes, combines and evaluates at zeta itself"""
        check(self._L.tmx_air_sha512_link_verify_device(self._h, C.byref(self._batch_params(params)), k_trace, k_helper, d_caps, d_proof, d_pub,
                                                        d_ok, self._stream(stream)), self._h)

    def trace_commit_set_air_sha512_link_device(self, section, d_pub, d_cap_h, d_cap_q, stream=None):
        """adds the SHA-512 link helper and quotient of the resident member `section` (SHA512 only) against the public table at d_pub to the
        commit set, behind the pairs of sets 7 - 9 that already follow the table"""
        check(self._L.tmx_trace_commit_set_air_sha512_link_device(self._h, section, d_pub, d_cap_h, d_cap_q, self._stream(stream)), self._h)

    def air_sha512_link_periodic_device(self, log_rows, log_blowup, d_pre, d_ext, stream=None):
        """STA, CHN, SEL, E79, MSG (planar, 5 << log_rows words at d_pre) and, unless log_blowup is 0, their extension under the current NTT
        domain at d_ext"""
        check(self._L.tmx_air_sha512_link_periodic_device(self._h, log_rows, log_blowup, d_pre, d_ext, self._stream(stream)), self._h)

    def air_sha512_link_periodic_eval_device(self, log_rows, d_zeta, d_out, stream=None):
        """d_out[0 .. 10) = the five planes at the F_p^2 point at d_zeta, barycentric over the 2^log_rows rows; d_out[10] = 1 on a zero
        denominator"""
        check(self._L.tmx_air_sha512_link_periodic_eval_device(self._h, log_rows, d_zeta, d_out, self._stream(stream)), self._h)

    def air_sha512_link_public_side_device(self, log_rows, log_blowup, n_proofs, d_pub, d_gamma, d_v, d_ext, stream=None):
        """V_r under the gamma at d_gamma (planar, 2 << log_rows words at d_v) and, unless log_blowup is 0, Pub_gamma on the coset at d_ext"""
        check(self._L.tmx_air_sha512_link_public_side_device(self._h, log_rows, log_blowup, n_proofs, d_pub, d_gamma, d_v, d_ext,
                                                             self._stream(stream)), self._h)

    def air_sha512_link_public_eval_device(self, log_rows, d_v, d_zeta, d_out, stream=None):
        """d_out[0 .. 2) = Pub_gamma at the F_p^2 point at d_zeta, barycentric over the 2^log_rows rows of V at d_v; d_out[2] = 1 on a zero
        denominator"""
        check(self._L.tmx_air_sha512_link_public_eval_device(self._h, log_rows, d_v, d_zeta, d_out, self._stream(stream)), self._h)

    def air_sha256_link_quotient_device(self, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper, d_pub, d_quot,
                                        stream=None, proof_range=None, accumulate=0):
        """gamma from the table cap, the helper cap and the digest of d_pub, the seventeen public polynomials, then the quotient of the 50
        constraints per proof over the extended table and helper columns into d_quot (planar, 2 << log_n words); proof_range and accumulate
        as in air_sha256_quotient_device: the piece that starts at proof 0 carries the public side"""
        if proof_range is not None or accumulate:
            lo, hi = proof_range if proof_range is not None else (0, n_proofs)
            check(self._L.tmx_air_sha256_link_quotient_range_device(self._h, log_n, log_blowup, cap_height, n_proofs, lo, hi, int(accumulate), d_cols,
                                                                    d_helper_cols, d_cap, d_cap_helper, d_pub, d_quot, self._stream(stream)), self._h)
            return
        check(self._L.tmx_air_sha256_link_quotient_device(self._h, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper,
                                                          d_pub, d_quot, self._stream(stream)), self._h)

    def air_sha256_link_verify_device(self, params, k_trace, k_helper, d_caps, d_proof, d_pub, d_ok, stream=None):
        """batch_verify_device, then the set-6 identity at zeta for the oracles k_trace (table), k_helper (helper), k_helper + 1 (quotient)
        against the public table at d_pub, which the verifier hashes and combines itself"""
        check(self._L.tmx_air_sha256_link_verify_device(self._h, C.byref(self._batch_params(params)), k_trace, k_helper, d_caps, d_proof, d_pub,
                                                        d_ok, self._stream(stream)), self._h)

    def trace_commit_set_air_sha256_link_device(self, section, d_pub, d_cap_h, d_cap_q, stream=None):
        """adds the link helper and quotient of the resident member `section` (SHA256, TREE or HEADER) against the public table at d_pub to
        the commit set, behind the last helper/quotient pair that already follows the table"""
        check(self._L.tmx_trace_commit_set_air_sha256_link_device(self._h, section, d_pub, d_cap_h, d_cap_q, self._stream(stream)), self._h)

    # ---- constraint set 7: the round constraints of the SHA-512 table (include/tmx.h)
    def air_sha512_helper_device(self, log_rows, n_proofs, d_table, d_helper, stream=None):
        """the helper oracle (599 n_proofs columns of 2^log_rows words at d_helper) from the pre-LDE T.2 columns (18 n_proofs) at d_table"""
        check(self._L.tmx_air_sha512_helper_device(self._h, log_rows, n_proofs, d_table, d_helper, self._stream(stream)), self._h)

    def air_sha512_quotient_device(self, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper, d_quot, stream=None,
                                   proof_range=None, accumulate=0):
        """the preprocessed columns filled and extended, gamma from the table cap and the helper cap, then the quotient of the 628 constraints
        per proof over the extended table and helper columns into d_quot (planar, 2 << log_n words); proof_range and accumulate as in
        air_sha256_quotient_device"""
        if proof_range is not None or accumulate:
            lo, hi = proof_range if proof_range is not None else (0, n_proofs)
            check(self._L.tmx_air_sha512_quotient_range_device(self._h, log_n, log_blowup, cap_height, n_proofs, lo, hi, int(accumulate), d_cols,
                                                               d_helper_cols, d_cap, d_cap_helper, d_quot, self._stream(stream)), self._h)
            return
        check(self._L.tmx_air_sha512_quotient_device(self._h, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper,
                                                     d_quot, self._stream(stream)), self._h)

    def air_sha512_verify_device(self, params, k_trace, d_caps, d_proof, d_ok, stream=None):
        """batch_verify_device, then the set-7 identity at zeta for the oracles k_trace (table), k_trace + 1 (helper), k_trace + 2 (quotient)"""
        check(self._L.tmx_air_sha512_verify_device(self._h, C.byref(self._batch_params(params)), k_trace, d_caps, d_proof, d_ok,
                                                   self._stream(stream)), self._h)

    def trace_commit_set_air_sha512_device(self, section, d_cap_h, d_cap_q, stream=None):
        """adds the SHA-512 helper and quotient of the resident member `section` (SHA512 only) to the commit set, directly behind it"""
        check(self._L.tmx_trace_commit_set_air_sha512_device(self._h, section, d_cap_h, d_cap_q, self._stream(stream)), self._h)

    def air_sha512_periodic_device(self, log_rows, log_blowup, d_pre, d_ext, stream=None):
        """SEL, KLO, KHI (3 << log_rows words at d_pre) and, unless log_blowup is 0, their extension under the current NTT domain at d_ext"""
        check(self._L.tmx_air_sha512_periodic_device(self._h, log_rows, log_blowup, d_pre, d_ext, self._stream(stream)), self._h)

    def air_sha512_periodic_eval_device(self, log_rows, d_zeta, d_out, stream=None):
        """d_out[0 .. 6) = SEL, KLO, KHI at the F_p^2 point at d_zeta, barycentric over the 2^log_rows rows; d_out[6] = 1 on a zero denominator"""
        check(self._L.tmx_air_sha512_periodic_eval_device(self._h, log_rows, d_zeta, d_out, self._stream(stream)), self._h)

    # ---- constraint set 8: the message schedule of the SHA-512 table (include/tmx.h)
    def air_sha512_sched_helper_device(self, log_rows, n_proofs, d_table, d_helper, stream=None):
        """the schedule helper (230 n_proofs columns of 2^log_rows words at d_helper) from the pre-LDE T.2 columns (18 n_proofs) at d_table"""
        check(self._L.tmx_air_sha512_sched_helper_device(self._h, log_rows, n_proofs, d_table, d_helper, self._stream(stream)), self._h)

    def air_sha512_sched_quotient_device(self, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper, d_quot,
                                         stream=None, proof_range=None, accumulate=0):
        """SCH filled and extended, gamma from the table cap and the helper cap, then the quotient of the 234 constraints per proof over the
        extended table and helper columns into d_quot (planar, 2 << log_n words); proof_range and accumulate as in
        air_sha256_quotient_device"""
        if proof_range is not None or accumulate:
            lo, hi = proof_range if proof_range is not None else (0, n_proofs)
            check(self._L.tmx_air_sha512_sched_quotient_range_device(self._h, log_n, log_blowup, cap_height, n_proofs, lo, hi, int(accumulate), d_cols,
                                                                     d_helper_cols, d_cap, d_cap_helper, d_quot, self._stream(stream)), self._h)
            return
        check(self._L.tmx_air_sha512_sched_quotient_device(self._h, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap,
                                                           d_cap_helper, d_quot, self._stream(stream)), self._h)

    def air_sha512_sched_verify_device(self, params, k_trace, k_helper, d_caps, d_proof, d_ok, stream=None):
        """batch_verify_device, then the set-8 identity at zeta for the oracles k_trace (table), k_helper (helper), k_helper + 1 (quotient)"""
        check(self._L.tmx_air_sha512_sched_verify_device(self._h, C.byref(self._batch_params(params)), k_trace, k_helper, d_caps, d_proof, d_ok,
                                                         self._stream(stream)), self._h)

    def trace_commit_set_air_sha512_sched_device(self, section, d_cap_h, d_cap_q, stream=None):
        """adds the SHA-512 schedule helper and quotient of the resident member `section` (SHA512 only) to the commit set, behind the table
        or behind set 7's pair"""
        check(self._L.tmx_trace_commit_set_air_sha512_sched_device(self._h, section, d_cap_h, d_cap_q, self._stream(stream)), self._h)

    def air_sha512_sched_periodic_device(self, log_rows, log_blowup, d_pre, d_ext, stream=None):
        """SCH (1 << log_rows words at d_pre) and, unless log_blowup is 0, its extension under the current NTT domain at d_ext"""
        check(self._L.tmx_air_sha512_sched_periodic_device(self._h, log_rows, log_blowup, d_pre, d_ext, self._stream(stream)), self._h)

    def air_sha512_sched_periodic_eval_device(self, log_rows, d_zeta, d_out, stream=None):
        """d_out[0 .. 2) = SCH at the F_p^2 point at d_zeta, barycentric over the 2^log_rows rows; d_out[2] = 1 on a zero denominator"""
        check(self._L.tmx_air_sha512_sched_periodic_eval_device(self._h, log_rows, d_zeta, d_out, self._stream(stream)), self._h)

    # ---- constraint set 9: the block starts of the SHA-512 table (include/tmx.h)
    def air_sha512_init_helper_device(self, log_rows, n_proofs, d_table, d_helper, stream=None):
        """the block-start helper (629 n_proofs columns of 2^log_rows words at d_helper) from the pre-LDE T.2 columns (18 n_proofs) at d_table"""
        check(self._L.tmx_air_sha512_init_helper_device(self._h, log_rows, n_proofs, d_table, d_helper, self._stream(stream)), self._h)

    def air_sha512_init_quotient_device(self, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap, d_cap_helper, d_quot,
                                        stream=None, proof_range=None, accumulate=0):
        """STA and CHN filled and extended, gamma from the table cap and the helper cap, then the quotient of the 673 constraints per proof
        over the extended table and helper columns into d_quot (planar, 2 << log_n words); proof_range and accumulate as in
        air_sha256_quotient_device"""
        if proof_range is not None or accumulate:
            lo, hi = proof_range if proof_range is not None else (0, n_proofs)
            check(self._L.tmx_air_sha512_init_quotient_range_device(self._h, log_n, log_blowup, cap_height, n_proofs, lo, hi, int(accumulate), d_cols,
                                                                    d_helper_cols, d_cap, d_cap_helper, d_quot, self._stream(stream)), self._h)
            return
        check(self._L.tmx_air_sha512_init_quotient_device(self._h, log_n, log_blowup, cap_height, n_proofs, d_cols, d_helper_cols, d_cap,
                                                          d_cap_helper, d_quot, self._stream(stream)), self._h)

    def air_sha512_init_verify_device(self, params, k_trace, k_helper, d_caps, d_proof, d_ok, stream=None):
        """batch_verify_device, then the set-9 identity at zeta for the oracles k_trace (table), k_helper (helper), k_helper + 1 (quotient)"""
        check(self._L.tmx_air_sha512_init_verify_device(self._h, C.byref(self._batch_params(params)), k_trace, k_helper, d_caps, d_proof, d_ok,
                                                        self._stream(stream)), self._h)

    def trace_commit_set_air_sha512_init_device(self, section, d_cap_h, d_cap_q, stream=None):
        """adds the SHA-512 block-start helper and quotient of the resident member `section` (SHA512 only) to the commit set, behind the
        table or behind the pairs of sets 7 and 8"""
        check(self._L.tmx_trace_commit_set_air_sha512_init_device(self._h, section, d_cap_h, d_cap_q, self._stream(stream)), self._h)

    def air_sha512_init_periodic_device(self, log_rows, log_blowup, d_pre, d_ext, stream=None):
        """STA, CHN (planar, 2 << log_rows words at d_pre) and, unless log_blowup is 0, their extension under the current NTT domain at d_ext"""
        check(self._L.tmx_air_sha512_init_periodic_device(self._h, log_rows, log_blowup, d_pre, d_ext, self._stream(stream)), self._h)

    def air_sha512_init_periodic_eval_device(self, log_rows, d_zeta, d_out, stream=None):
        """d_out[0 .. 4) = STA, CHN at the F_p^2 point at d_zeta, barycentric over the 2^log_rows rows; d_out[4] = 1 on a zero denominator"""
        check(self._L.tmx_air_sha512_init_periodic_eval_device(self._h, log_rows, d_zeta, d_out, self._stream(stream)), self._h)

    # ---- streamed helpers of constraint sets 3 - 5 (include/tmx.h "streamed helpers of the SHA-256 sets")
    def trace_commit_set_air_sha256_streamed_device(self, constraint_set, section, chunk_proofs, d_cap_h, d_cap_q, stream=None):
        """the set-level call of constraint set 3, 4 or 5 with the helper fed in chunks of chunk_proofs whole proofs and never resident
        extended: the same caps, gamma, shape and proof words as the resident call"""
        check(self._L.tmx_trace_commit_set_air_sha256_streamed_device(self._h, constraint_set, section, chunk_proofs, d_cap_h, d_cap_q,
                                                                      self._stream(stream)), self._h)

    def trace_commit_set_air_sha256_scratch_bytes(self, constraint_set, section):
        """(host only) the bytes of the scratch the context holds for that set and section right now; 0 if none"""
        return int(self._L.tmx_trace_commit_set_air_sha256_scratch_bytes(self._h, constraint_set, section))

    # ---- streamed helpers of constraint sets 7 - 9 (include/tmx.h "streamed helpers of the SHA-512 sets")
    def trace_commit_set_air_sha512_streamed_device(self, constraint_set, section, chunk_proofs, d_cap_h, d_cap_q, stream=None):
        """the set-level call of constraint set 7, 8 or 9 on TRACE_SHA512 with the helper fed in chunks of chunk_proofs whole proofs and
        never resident extended: the same caps, gamma, shape and proof words as the resident call"""
        check(self._L.tmx_trace_commit_set_air_sha512_streamed_device(self._h, constraint_set, section, chunk_proofs, d_cap_h, d_cap_q,
                                                                      self._stream(stream)), self._h)

    def trace_commit_set_air_sha512_scratch_bytes(self, constraint_set, section):
        """(host only) the bytes of the scratch the context holds for set 7, 8 or 9 on that section right now; 0 if none"""
        return int(self._L.tmx_trace_commit_set_air_sha512_scratch_bytes(self._h, constraint_set, section))

    # ---- multi-GPU: the RCCL exchange behind the C ABI (include/tmx.h "multi-GPU")
    def comm_create(self, unique_id, rank, world):
        check(self._L.tmx_comm_create(self._h, bytes(unique_id) if unique_id is not None else None, rank, world), self._h)

    def comm_destroy(self):
        check(self._L.tmx_comm_destroy(self._h), self._h)

    def comm_abort(self):
        check(self._L.tmx_comm_abort(self._h), self._h)

    def comm_sync(self, stream=None, timeout_ms=0):
        """Bounded wait for `stream` after a sharded call: TmxError(-7) if a peer aborted / died or the timeout passed (include/tmx.h FAILURE CONTRACT)."""
        check(self._L.tmx_comm_sync(self._h, self._stream(stream), int(timeout_ms)), self._h)

    def comm_info(self):
        r, w = C.c_uint32(), C.c_uint32()
        check(self._L.tmx_comm_info(self._h, C.byref(r), C.byref(w)), self._h)
        return r.value, w.value

    def witness_batch_sharded_device(self, kind, n_total, d_proofs, d_targets, d_trusteds, d_out, d_reports, gather=False, stream=None):
        check(self._L.tmx_witness_batch_sharded_device(self._h, kind, n_total, d_proofs, d_targets, d_trusteds, d_out, d_reports,
                                                       1 if gather else 0, self._stream(stream)), self._h)

    def witness_validator_sharded_device(self, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out, d_reports, stream=None):
        check(self._L.tmx_witness_validator_sharded_device(self._h, kind, n_proofs, d_proofs, d_targets, d_trusteds, d_out, d_reports,
                                                           self._stream(stream)), self._h)

    def trace_rows_sharded_device(self, kind, n_total, d_targets, d_trusteds, d_trace_out, sections=_lib.TRACE_ALL, gather=False, stream=None):
        """Level-2 rows of this rank's proofs of a proof-sharded batch (after witness_batch_sharded_device of the same n_total); gather: all rows everywhere."""
        check(self._L.tmx_trace_rows_sharded_device(self._h, kind, n_total, d_targets, d_trusteds, d_trace_out, sections, 1 if gather else 0,
                                                    self._stream(stream)), self._h)

    def trace_rows_validator_sharded_device(self, kind, n_proofs, d_targets, d_trusteds, d_trace_out, sections=_lib.TRACE_ALL, stream=None):
        """Level-2 rows with the per-lane sections (ladders, SHA-512) lane-sharded and exchanged (after witness_validator_sharded_device)."""
        check(self._L.tmx_trace_rows_validator_sharded_device(self._h, kind, n_proofs, d_targets, d_trusteds, d_trace_out, sections, self._stream(stream)), self._h)

    def trace_commit_sharded_device(self, kind, n_total, section, log_blowup, cap_height, d_trace_rows, d_caps, stream=None):
        check(self._L.tmx_trace_commit_sharded_device(self._h, kind, n_total, section, log_blowup, cap_height, d_trace_rows, d_caps, self._stream(stream)), self._h)

    def last_kernel_ms(self):
        ms = (C.c_float * _lib.N_KERNELS)()
        check(self._L.tmx_last_kernel_ms(self._h, ms), self._h)
        return dict(zip(_lib.KERNEL_NAMES, (float(x) for x in ms)))

    def kernel_ms_mean(self, last_k):
        """Mean HIP-event duration per kernel over the last `last_k` enqueued batches (blocks until they finished)."""
        ms = (C.c_float * _lib.N_KERNELS)()
        check(self._L.tmx_kernel_ms_mean(self._h, last_k, ms), self._h)
        return dict(zip(_lib.KERNEL_NAMES, (float(x) for x in ms)))

    def last_dedup(self):
        """(distinct public keys, table path used) of the last EdDSA launch."""
        u, t = C.c_uint32(), C.c_uint32()
        check(self._L.tmx_last_dedup(self._h, C.byref(u), C.byref(t)), self._h)
        return int(u.value), bool(t.value)

    def last_proof_path(self):
        """Which launch computed the proof-level values of the last batch (tmx_last_proof_path): one of _lib.PROOF_PATH_*.  Host-side, does not block."""
        path = int(self._L.tmx_last_proof_path(self._h))
        if path < 0:
            check(path, self._h)
        return path

    # ---- persistent per-key table cache (tmx_key_cache_*)
    def key_cache_stats(self):
        info = _lib.KeyCacheInfo()
        check(self._L.tmx_key_cache_stats(self._h, C.byref(info)), self._h)
        return info.as_dict()

    def set_cache_stats(self):
        """The validator-set cache (tmx_set_cache_stats): sets resident / served from the cache / computed / inserted / evicted (LRU), capacity."""
        out = (C.c_uint32 * 8)()
        check(self._L.tmx_set_cache_stats(self._h, out), self._h)
        return dict(zip(("resident", "served", "computed", "inserted", "evicted", "capacity"), (int(x) for x in out)))

    def key_cache_flush(self):
        check(self._L.tmx_key_cache_flush(self._h), self._h)

    def key_cache_config(self, enabled=True, max_keys=0):
        """enabled=False: tables do not survive a call (every call cold); max_keys != 0: new capacity (flushes)."""
        check(self._L.tmx_key_cache_config(self._h, 1 if enabled else 0, int(max_keys)), self._h)

    def sync(self):
        check(self._L.tmx_sync(self._h), self._h)


def fri_layout(params, L=None):
    """tmx_fri_layout_of as a dict (no context, no device): n_layers, final_log, layer_bits, layer_cap_height, off_caps, off_final,
    off_indices, off_init_rows, off_init_paths, off_rows, off_paths, words"""
    L = L or _lib.lib()
    out = _lib.FriLayout()
    check(L.tmx_fri_layout_of(C.byref(Context._fri_params(params)), C.byref(out)))
    n = out.n_layers
    return {"n_layers": n, "final_log": out.final_log, "layer_bits": list(out.layer_bits[:n]), "layer_cap_height": list(out.layer_cap_height[:n]),
            "off_caps": list(out.off_caps[:n]), "off_final": out.off_final, "off_indices": out.off_indices, "off_init_rows": out.off_init_rows,
            "off_init_paths": out.off_init_paths, "off_rows": list(out.off_rows[:n]), "off_paths": list(out.off_paths[:n]), "words": out.words}


def deep_openings_words(n_cols, L=None):
    """tmx_deep_openings_words: 4 R words (R = n_cols rounded up to a power of two), 0 for n_cols 0 or above 2^24"""
    L = L or _lib.lib()
    return int(L.tmx_deep_openings_words(int(n_cols)))


def deep_proof_words(params, L=None):
    """the words of a DEEP proof: the openings section, then the FRI proof of the same parameters; TmxError on parameters the DEEP calls
    refuse (FRI's rules and n_cols <= 2^24)"""
    p = Context._fri_params(params)
    fri_words = fri_layout(p, L)["words"]
    open_words = deep_openings_words(p.n_cols, L)
    if not open_words:
        raise _lib.TmxError(-1, "n_cols must be at most 2^24 for a DEEP proof")
    return open_words + fri_words


def pow_proof_words(params, pow_bits, deep=False, L=None):
    """tmx_pow_proof_words: the words of a grinding proof (the FRI or DEEP proof, then the nonce); TmxError on parameters the calls refuse"""
    L = L or _lib.lib()
    words = int(L.tmx_pow_proof_words(C.byref(Context._pow_params(params, pow_bits, deep))))
    if not words:
        raise _lib.TmxError(-1, "parameters refused: the rules of the underlying proof, 1 <= pow_bits <= 24, deep 0 or 1")
    return words


def batch_layout(params, L=None):
    """tmx_batch_layout_of as a dict (no context, no device); TmxError on parameters the ABI refuses"""
    L = L or _lib.lib()
    p = Context._batch_params(params)
    out = _lib.BatchLayout()
    check(L.tmx_batch_layout_of(C.byref(p), C.byref(out)))
    n, K = out.n_layers, p.n_oracles
    return {"n_layers": n, "final_log": out.final_log, "n_groups": out.n_groups, "layer_bits": list(out.layer_bits[:n]),
            "layer_cap_height": list(out.layer_cap_height[:n]), "layer_enter": list(out.layer_enter[:n]), "group_of": list(out.group_of[:K]),
            "cap_height_of": list(out.cap_height_of[:K]), "off_open": list(out.off_open[:K]), "off_caps": list(out.off_caps[:n]),
            "off_final": out.off_final, "off_indices": out.off_indices, "off_init_rows": list(out.off_init_rows[:K]),
            "off_init_paths": list(out.off_init_paths[:K]), "off_rows": list(out.off_rows[:n]), "off_paths": list(out.off_paths[:n]),
            "off_nonce": out.off_nonce, "words": out.words}


def trace_commit_set_bytes(kind, n_max, n_proofs, sections, streamed, chunk_cols, log_blowup, cap_height, L=None):
    """tmx_trace_commit_set_bytes (no context, no device): set scratch + LDE scratch of a commit set in bytes; 0 for arguments the commit
    would refuse"""
    L = L or _lib.lib()
    return int(L.tmx_trace_commit_set_bytes(kind, n_max, n_proofs, sections, streamed, chunk_cols, log_blowup, cap_height))


def trace_commit_set_air_sha256_streamed_bytes(constraint_set, log_m, log_blowup, cap_height, n_proofs, chunk_proofs, L=None):
    """tmx_trace_commit_set_air_sha256_streamed_bytes (no context, no device): (scratch bytes of the streamed set-level call, the LDE's own
    scratch in bytes); (0, 0) for a refused shape"""
    L = L or _lib.lib()
    lde = C.c_uint64(0)
    return int(L.tmx_trace_commit_set_air_sha256_streamed_bytes(constraint_set, log_m, log_blowup, cap_height, n_proofs, chunk_proofs,
                                                                 C.byref(lde))), int(lde.value)


def trace_commit_set_air_sha512_streamed_bytes(constraint_set, log_m, log_blowup, cap_height, n_proofs, chunk_proofs, L=None):
    """tmx_trace_commit_set_air_sha512_streamed_bytes (no context, no device): (scratch bytes of the streamed set-level call of set 7, 8 or
    9, the LDE's own scratch in bytes); (0, 0) for a refused shape"""
    L = L or _lib.lib()
    lde = C.c_uint64(0)
    return int(L.tmx_trace_commit_set_air_sha512_streamed_bytes(constraint_set, log_m, log_blowup, cap_height, n_proofs, chunk_proofs,
                                                                 C.byref(lde))), int(lde.value)


def air_sha256_public_shape(kind, section, n_max, n_proofs, L=None):
    """tmx_air_sha256_public_shape (no context, no device): (log2 K, columns) of the public table of constraint set 6"""
    L = L or _lib.lib()
    log_k, n_cols = C.c_uint32(), C.c_uint32()
    check(L.tmx_air_sha256_public_shape(kind, section, n_max, n_proofs, C.byref(log_k), C.byref(n_cols)))
    return int(log_k.value), int(n_cols.value)


def air_sha512_public_shape(kind, n_max, n_proofs, L=None):
    """tmx_air_sha512_public_shape (no context, no device): (log2 K, columns) of the public table of constraint set 10"""
    L = L or _lib.lib()
    log_k, n_cols = C.c_uint32(), C.c_uint32()
    check(L.tmx_air_sha512_public_shape(kind, n_max, n_proofs, C.byref(log_k), C.byref(n_cols)))
    return int(log_k.value), int(n_cols.value)


def air_ladder_public_shape(kind, n_max, n_proofs, L=None):
    """tmx_air_ladder_public_shape (no context, no device): (log2 K, columns) of the public table of constraint set 2"""
    L = L or _lib.lib()
    log_k, n_cols = C.c_uint32(), C.c_uint32()
    check(L.tmx_air_ladder_public_shape(kind, n_max, n_proofs, C.byref(log_k), C.byref(n_cols)))
    return int(log_k.value), int(n_cols.value)
