"""Loader and thin object wrappers for csrc/libmi355nrphy.so (the C ABI of include/mi355_nrphy.h).

There is deliberately no CPU implementation behind these classes: if the HIP library is missing or no GPU is
present the constructors raise.  PyTorch is used only as the device-memory allocator / stream provider of the
callers (tests, bench.py): tensors are passed down as raw device pointers.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
# NRPHY_LIB_SO: another build of the same library (A/B variants, the host-sanitizer build of profiles/sanitize_cpu.sh)
LIB_PATH = os.environ.get("NRPHY_LIB_SO") or os.path.join(HERE, "csrc", "libmi355nrphy.so")

_LIB = None


class NrphyError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        super().__init__("%s failed: status %d (%s)" % (what, status, strerror(status)))


def load():
    """Returns the ctypes handle of libmi355nrphy.so; raises if it has not been built."""
    global _LIB
    if _LIB is None:
        try:
            # PyTorch bundles its own HIP runtime; let it load first so that this library binds to the same
            # libamdhip64 instead of bringing a second runtime into the process (device memory comes from torch).
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("HIP library %s is missing: run `python srsran-edgeric-5g_amd/build.py` "
                               "(there is no CPU fallback)" % LIB_PATH)
        _LIB = abi.declare(C.CDLL(LIB_PATH))
    return _LIB


def strerror(status):
    return load().nrphy_strerror(status).decode()


def _check(status, what):
    if status != abi.OK:
        raise NrphyError(status, what)


# Callers that order their PyTorch work and this library's streams themselves (bench.py: explicit synchronisation around the timed
# region) switch the wait below off.
ORDER_AFTER_TORCH = True


def _stream(stream):
    """The stream argument of a device entry point.  None selects the context's own stream, which is non-blocking and therefore
    NOT ordered after PyTorch's streams: work PyTorch has queued on its current stream (the fill of a fresh torch.zeros, a
    host-to-device copy) is waited for first, so that a tensor handed over is what the caller sees.  An explicit stream is the
    caller's to order."""
    if stream is None and ORDER_AFTER_TORCH:
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available():
            torch.cuda.current_stream().synchronize()
    return stream


def _dptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


class Context:
    """nrphy_ctx: device tables + default stream.  Replaces the reference's factory chain."""

    def __init__(self, device_id=0):
        self.lib = load()
        h = C.c_void_p()
        _check(self.lib.nrphy_create(C.byref(h), device_id), "nrphy_create")
        self.handle = h
        self.device_id = device_id

    def close(self):
        if self.handle:
            self.lib.nrphy_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self, stream=None):
        _check(self.lib.nrphy_synchronize(self.handle, stream), "nrphy_synchronize")

    # ---- single-PDU host-span entry points (reference semantics) --------------------------------------
    def pdsch_process_host(self, pdu, tb, nof_ports, nof_subc, grid=None, taps=False):
        """pdsch_processor::process with host spans.  Returns grid [ports][14][subc][2] uint16 (raw bf16)
        and, with taps, the packed rate-matched and scrambled codewords."""
        tb = np.ascontiguousarray(tb, dtype=np.uint8)
        if grid is None:
            grid = np.zeros((nof_ports, 14, nof_subc, 2), np.uint16)
        d = derive(pdu)
        nb = (d["codeword_bits"] + 7) // 8
        rm = np.zeros(nb, np.uint8) if taps else None
        scr = np.zeros(nb, np.uint8) if taps else None
        _check(self.lib.nrphy_pdsch_process_host(
            self.handle, C.byref(pdu), tb.ctypes.data, grid.ctypes.data, nof_ports, nof_subc,
            rm.ctypes.data if taps else None, scr.ctypes.data if taps else None), "nrphy_pdsch_process_host")
        return (grid, rm, scr) if taps else grid

    def pdsch_encode_host(self, base_graph, rv, qm, nref, nof_layers, nof_ch_symbols, tb):
        """pdsch_encoder::encode: returns (codeword bits one per byte, the same packed MSB-first)."""
        tb = np.ascontiguousarray(tb, dtype=np.uint8)
        cfg = abi.PdschEncoderCfg(base_graph, rv, qm, nref, nof_layers, nof_ch_symbols, tb.size)
        bits = np.zeros(nof_ch_symbols * qm, np.uint8)
        packed = np.zeros((bits.size + 7) // 8, np.uint8)
        _check(self.lib.nrphy_pdsch_encode_host(self.handle, C.byref(cfg), tb.ctypes.data, bits.ctypes.data,
                                                packed.ctypes.data), "nrphy_pdsch_encode_host")
        return bits, packed

    def ldpc_encode(self, base_graph, lifting_size, d_msg, msg_stride, out_bits, d_out, out_stride, n_cb, stream=None):
        _check(self.lib.nrphy_ldpc_encode(self.handle, base_graph, lifting_size, n_cb, _dptr(d_msg), msg_stride,
                                          out_bits, _dptr(d_out), out_stride, _stream(stream)), "nrphy_ldpc_encode")

    def ldpc_rate_dematch(self, cfg, n_cb, d_in, in_stride, d_soft, soft_stride, new_data, stream=None):
        """ldpc_rate_dematcher::rate_dematch for n_cb codeblocks resident in HBM (cfg: abi.LdpcRateDematcherCfg)."""
        _check(self.lib.nrphy_ldpc_rate_dematch(self.handle, C.byref(cfg), n_cb, _dptr(d_in), in_stride, _dptr(d_soft),
                                                soft_stride, int(new_data), _stream(stream)), "nrphy_ldpc_rate_dematch")

    def ldpc_rate_dematch_host(self, base_graph, lifting_size, rv, qm, nref, nof_filler, new_data, llr_in, soft_buffer):
        """ldpc_rate_dematcher::rate_dematch on host spans: returns the updated soft buffer (copy)."""
        llr_in = np.ascontiguousarray(llr_in, dtype=np.int8)
        out = np.array(soft_buffer, dtype=np.int8, copy=True)
        cfg = abi.LdpcRateDematcherCfg(base_graph, lifting_size, rv, qm, nref, nof_filler, llr_in.size)
        _check(self.lib.nrphy_ldpc_rate_dematch_host(self.handle, C.byref(cfg), llr_in.ctypes.data, out.ctypes.data,
                                                     int(new_data)), "nrphy_ldpc_rate_dematch_host")
        return out

    def pusch_decode_codeblock_host(self, base_graph, lifting_size, rv, qm, nref, nof_filler, crc_poly, max_iterations,
                                    scaling, new_data, llr_in, soft_buffer):
        """Rate dematcher + decoder of one codeblock on host spans (the hw_accelerator_pusch_dec operation):
        returns (iterations or 0, Kb*Zc hard bits, updated soft buffer)."""
        llr_in = np.ascontiguousarray(llr_in, dtype=np.int8)
        soft = np.array(soft_buffer, dtype=np.int8, copy=True)
        cfg = abi.LdpcRateDematcherCfg(base_graph, lifting_size, rv, qm, nref, nof_filler, llr_in.size)
        k = (22 if base_graph == 1 else 10) * lifting_size
        packed = np.zeros((k + 7) // 8, np.uint8)
        it = C.c_uint32(0)
        _check(self.lib.nrphy_pusch_decode_codeblock_host(self.handle, C.byref(cfg), crc_poly, max_iterations, scaling,
                                                          llr_in.ctypes.data, soft.ctypes.data, int(new_data),
                                                          packed.ctypes.data, C.byref(it)),
               "nrphy_pusch_decode_codeblock_host")
        return int(it.value), np.unpackbits(packed)[:k], soft

    def llr_descramble(self, d_c_init, n_cw, length, d_in, in_stride, d_out, out_stride, stream=None):
        """pseudo_random_generator::apply_xor on soft bits for n_cw codewords in device memory (d_c_init: device uint32)."""
        _check(self.lib.nrphy_llr_descramble(self.handle, n_cw, _dptr(d_c_init), length, _dptr(d_in), in_stride, _dptr(d_out),
                                             out_stride, _stream(stream)), "nrphy_llr_descramble")

    def llr_descramble_host(self, c_init, llr):
        """One codeword of int8 soft bits from host memory; returns the descrambled copy."""
        llr = np.ascontiguousarray(llr, dtype=np.int8)
        out = np.empty_like(llr)
        _check(self.lib.nrphy_llr_descramble_host(self.handle, c_init, llr.size, llr.ctypes.data, out.ctypes.data),
               "nrphy_llr_descramble_host")
        return out

    def pdsch_process_slot_host(self, pdus, tbs, grid):
        """All PDSCH PDUs of one slot into one host grid [nof_ports][14][nof_subc][2] uint16 (read first, written back)."""
        n = len(pdus)
        arr = (abi.PdschPdu * n)(*pdus)
        keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in tbs]
        ptrs = (C.c_void_p * n)(*[t.ctypes.data for t in keep])
        grid = np.ascontiguousarray(grid, dtype=np.uint16)
        _check(self.lib.nrphy_pdsch_process_slot_host(self.handle, n, arr, ptrs, grid.ctypes.data, grid.shape[0], grid.shape[2]),
               "nrphy_pdsch_process_slot_host")
        return grid

    def demodulate_soft(self, modulation, nof_spans, span_len, d_symbols, d_noise_vars, d_llr, stream=None):
        """demodulation_mapper::demodulate_soft for nof_spans spans of span_len symbols in device memory."""
        _check(self.lib.nrphy_demodulate_soft(self.handle, modulation, nof_spans, span_len, _dptr(d_symbols), _dptr(d_noise_vars),
                                              _dptr(d_llr), _stream(stream)), "nrphy_demodulate_soft")

    def demodulate_soft_host(self, modulation, symbols, noise_vars):
        """One span from host memory: symbols complex64 [n], noise_vars float32 [n] -> int8 [n * bits per symbol]."""
        symbols = np.ascontiguousarray(symbols, dtype=np.complex64)
        noise_vars = np.ascontiguousarray(noise_vars, dtype=np.float32)
        assert symbols.size == noise_vars.size
        out = np.zeros(symbols.size * max(modulation, 1), np.int8)
        _check(self.lib.nrphy_demodulate_soft_host(self.handle, modulation, symbols.size, symbols.ctypes.data,
                                                   noise_vars.ctypes.data, out.ctypes.data), "nrphy_demodulate_soft_host")
        return out

    def grid_put(self, d_grid, nof_ports, nof_subc, entries, stream=None):
        """Sparse host writes into ONE device grid: entries = [(port, symbol, subc, cbf16 word)], later ones win."""
        n = len(entries)
        arr = (abi.GridRe * n)(*[abi.GridRe(*e) for e in entries])
        _check(self.lib.nrphy_grid_put(self.handle, _dptr(d_grid), nof_ports, nof_subc, n, arr, _stream(stream)), "nrphy_grid_put")

    def csi_rs_map(self, cfgs, grid_indices, d_grid, nof_ports, nof_subc, stream=None):
        """nzp_csi_rs_generator::map for a batch of signals into device grids [grid][port][14][subc]."""
        n = len(cfgs)
        arr = (abi.CsiRsCfg * n)(*cfgs)
        idx = (C.c_uint32 * n)(*grid_indices)
        _check(self.lib.nrphy_csi_rs_map(self.handle, n, arr, idx, _dptr(d_grid), nof_ports, nof_subc, _stream(stream)),
               "nrphy_csi_rs_map")

    def csi_rs_map_host(self, cfg, grid):
        """nzp_csi_rs_generator::map into a copy of a host grid [nof_ports][14][nof_subc][2] uint16 (raw cbf16)."""
        out = np.array(grid, dtype=np.uint16, copy=True)
        _check(self.lib.nrphy_csi_rs_map_host(self.handle, C.byref(cfg), out.ctypes.data, out.shape[0], out.shape[2]),
               "nrphy_csi_rs_map_host")
        return out

    # ---- downlink control channels (pdcch_processor, ssb_processor) --------------------------------------------
    def pdcch_process(self, pdus, grid_indices, d_grid, nof_ports, nof_subc, stream=None):
        """pdcch_processor::process for a batch of DCIs into device grids [grid][port][14][subc]."""
        n = len(pdus)
        arr = (abi.PdcchPdu * n)(*pdus)
        idx = (C.c_uint32 * n)(*grid_indices)
        _check(self.lib.nrphy_pdcch_process(self.handle, n, arr, idx, _dptr(d_grid), nof_ports, nof_subc, _stream(stream)),
               "nrphy_pdcch_process")

    def pdcch_process_host(self, pdu, grid):
        """pdcch_processor::process into a copy of a host grid [nof_ports][14][nof_subc][2] uint16 (raw cbf16)."""
        out = np.array(grid, dtype=np.uint16, copy=True)
        _check(self.lib.nrphy_pdcch_process_host(self.handle, C.byref(pdu), out.ctypes.data, out.shape[0], out.shape[2]),
               "nrphy_pdcch_process_host")
        return out

    def pdcch_encode_host(self, payload_bits, rnti, rm_length):
        """pdcch_encoder::encode: payload bits (one per byte) -> rm_length bits (one per byte)."""
        payload = np.ascontiguousarray(payload_bits, dtype=np.uint8)
        out = np.zeros(rm_length, np.uint8)
        _check(self.lib.nrphy_pdcch_encode_host(self.handle, payload.ctypes.data, payload.size, rnti, rm_length,
                                                out.ctypes.data), "nrphy_pdcch_encode_host")
        return out

    def ssb_process(self, pdus, grid_indices, d_grid, nof_ports, nof_subc, stream=None):
        """ssb_processor::process for a batch of SS/PBCH blocks into device grids [grid][port][14][subc]."""
        n = len(pdus)
        arr = (abi.SsbPdu * n)(*pdus)
        idx = (C.c_uint32 * n)(*grid_indices)
        _check(self.lib.nrphy_ssb_process(self.handle, n, arr, idx, _dptr(d_grid), nof_ports, nof_subc, _stream(stream)),
               "nrphy_ssb_process")

    def ssb_process_host(self, pdu, grid):
        """ssb_processor::process into a copy of a host grid [nof_ports][14][nof_subc][2] uint16 (raw cbf16)."""
        out = np.array(grid, dtype=np.uint16, copy=True)
        _check(self.lib.nrphy_ssb_process_host(self.handle, C.byref(pdu), out.ctypes.data, out.shape[0], out.shape[2]),
               "nrphy_ssb_process_host")
        return out

    def pbch_encode_host(self, pdu):
        """pbch_encoder::encode: the 864 rate-matched PBCH bits (one per byte)."""
        out = np.zeros(864, np.uint8)
        _check(self.lib.nrphy_pbch_encode_host(self.handle, C.byref(pdu), out.ctypes.data), "nrphy_pbch_encode_host")
        return out

    # ---- lower-PHY tail (amplitude controller, radio sample format, fronthaul compression) ------------------------
    def amplitude_control(self, cfg, n_buffers, nof_samples, d_in, d_out, d_stats=None, in_stride=None, out_stride=None,
                          stream=None):
        """amplitude_controller::process for n_buffers device buffers of nof_samples complex floats."""
        _check(self.lib.nrphy_amplitude_control(self.handle, C.byref(cfg), n_buffers, nof_samples, _dptr(d_in),
                                                in_stride or nof_samples, _dptr(d_out), out_stride or nof_samples,
                                                _dptr(d_stats), _stream(stream)), "nrphy_amplitude_control")

    def amplitude_control_host(self, cfg, x, metrics=None):
        """One host buffer (complex64) -> (output, abi.AmplitudeMetrics updated in place when given)."""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        out = np.zeros_like(x)
        m = metrics if metrics is not None else abi.AmplitudeMetrics()
        _check(self.lib.nrphy_amplitude_control_host(self.handle, C.byref(cfg), x.ctypes.data, x.size, out.ctypes.data,
                                                     C.byref(m)), "nrphy_amplitude_control_host")
        return out, m

    def iq_convert_ci16_host(self, x, scale):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        out = np.zeros(2 * x.size, np.int16)
        _check(self.lib.nrphy_iq_convert_ci16_host(self.handle, x.ctypes.data, x.size, scale, out.ctypes.data),
               "nrphy_iq_convert_ci16_host")
        return out

    def iq_convert_ci16(self, n_buffers, nof_samples, d_in, scale, d_out, in_stride=None, out_stride=None, stream=None):
        _check(self.lib.nrphy_iq_convert_ci16(self.handle, n_buffers, nof_samples, _dptr(d_in), in_stride or nof_samples,
                                              scale, _dptr(d_out), out_stride or nof_samples, _stream(stream)), "nrphy_iq_convert_ci16")

    def ofh_compress_host(self, cfg, prbs):
        """iq_compressor::compress + serialisation: prbs [nof_prb][12][2] uint16 (raw cbf16) -> bytes."""
        prbs = np.ascontiguousarray(prbs, dtype=np.uint16)
        nof_prb = prbs.size // 24
        out = np.zeros(nof_prb * self.lib.nrphy_ofh_compressed_prb_bytes(C.byref(cfg)), np.uint8)
        _check(self.lib.nrphy_ofh_compress_host(self.handle, C.byref(cfg), nof_prb, prbs.ctypes.data, out.ctypes.data),
               "nrphy_ofh_compress_host")
        return out

    def ofh_compress(self, cfg, n_rows, nof_prb, d_prbs, d_out, row_stride=None, out_row_stride=None, stream=None):
        rec = self.lib.nrphy_ofh_compressed_prb_bytes(C.byref(cfg))
        _check(self.lib.nrphy_ofh_compress(self.handle, C.byref(cfg), n_rows, nof_prb, _dptr(d_prbs), row_stride or 12 * nof_prb,
                                           _dptr(d_out), out_row_stride or rec * nof_prb, _stream(stream)), "nrphy_ofh_compress")

    def ofh_decompress_host(self, cfg, data):
        """iq_decompressor::decompress on serialised records: bytes -> prbs [nof_prb][12][2] uint16 (raw cbf16)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        nof_prb = data.size // self.lib.nrphy_ofh_compressed_prb_bytes(C.byref(cfg))
        out = np.zeros((nof_prb, 12, 2), np.uint16)
        _check(self.lib.nrphy_ofh_decompress_host(self.handle, C.byref(cfg), nof_prb, data.ctypes.data, out.ctypes.data),
               "nrphy_ofh_decompress_host")
        return out

    def ofh_decompress(self, cfg, n_rows, nof_prb, d_in, d_prbs, in_row_stride=None, row_stride=None, stream=None):
        """d_in: a device pointer (int) or a tensor -- the records may start at any byte."""
        rec = self.lib.nrphy_ofh_compressed_prb_bytes(C.byref(cfg))
        d_in = C.c_void_p(d_in) if isinstance(d_in, int) else _dptr(d_in)
        _check(self.lib.nrphy_ofh_decompress(self.handle, C.byref(cfg), n_rows, nof_prb, d_in, in_row_stride or rec * nof_prb,
                                             _dptr(d_prbs), row_stride or 12 * nof_prb, _stream(stream)), "nrphy_ofh_decompress")

    def ofh_ul_write_grid(self, sections, d_payload, d_grid, nof_grids, grid_nof_ports, grid_nof_subc, payload_bytes=None, stream=None):
        """sections: a list of abi.OfhUlSection; d_payload: a uint8 tensor; returns the status (NRPHY_OK or NRPHY_ERR_ARGUMENT)."""
        arr = (abi.OfhUlSection * max(len(sections), 1))(*sections)
        payload_bytes = d_payload.numel() if payload_bytes is None else payload_bytes
        return self.lib.nrphy_ofh_ul_write_grid(self.handle, len(sections), arr, _dptr(d_payload), payload_bytes, _dptr(d_grid), nof_grids,
                                                grid_nof_ports, grid_nof_subc, _stream(stream))

    def ofh_dl_write_frames(self, flows, symbols, d_grid, nof_grids, grid_nof_ports, grid_nof_subc, d_frames, frame_stride,
                            frames_bytes=None, stream=None):
        """flows: a list of abi.OfhDlFlow; symbols: a list of abi.OfhDlSymbol; d_frames: a uint8 tensor; returns the status."""
        f_arr = (abi.OfhDlFlow * max(len(flows), 1))(*flows)
        s_arr = (abi.OfhDlSymbol * max(len(symbols), 1))(*symbols)
        frames_bytes = d_frames.numel() * d_frames.element_size() if frames_bytes is None else frames_bytes
        return self.lib.nrphy_ofh_dl_write_frames(self.handle, len(flows), f_arr, len(symbols), s_arr, _dptr(d_grid), nof_grids,
                                                  grid_nof_ports, grid_nof_subc, _dptr(d_frames), frames_bytes, frame_stride,
                                                  _stream(stream))

    def ofh_dl_frames_host(self, flow, symbol, row, frames, frame_stride):
        """One symbol's row (raw cbf16, uint16 [nof_subc][2]) into the uint8 array `frames` in place; returns the status."""
        row = np.ascontiguousarray(row, dtype=np.uint16)
        assert frames.dtype == np.uint8 and frames.flags.c_contiguous
        return self.lib.nrphy_ofh_dl_frames_host(self.handle, C.byref(flow), C.byref(symbol), row.ctypes.data, row.size // 2,
                                                 frames.ctypes.data, frames.size, frame_stride)

    def ofh_ul_write_prach(self, sections, d_payload, d_symbols, symbols_elems, payload_bytes=None, stream=None):
        """sections: a list of abi.OfhUlPrachSection; d_symbols: the PRACH buffer, complex float; returns the status."""
        arr = (abi.OfhUlPrachSection * max(len(sections), 1))(*sections)
        payload_bytes = d_payload.numel() if payload_bytes is None else payload_bytes
        return self.lib.nrphy_ofh_ul_write_prach(self.handle, len(sections), arr, _dptr(d_payload), payload_bytes, _dptr(d_symbols),
                                                 symbols_elems, _stream(stream))

    def pusch_decoder_sizes(self, cfg, n_tb):
        """(soft-buffer bytes per transport block, state bytes of the batch, codeblocks per transport block)."""
        soft, state, scratch, ncb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        _check(self.lib.nrphy_pusch_decoder_sizes(self.handle, C.byref(cfg), n_tb, C.byref(soft), C.byref(state),
                                                  C.byref(scratch), C.byref(ncb)), "nrphy_pusch_decoder_sizes")
        self._pusch_scratch_bytes = int(scratch.value)
        return int(soft.value), int(state.value), int(ncb.value)

    def _scratch(self, nbytes, d_scratch):
        """The decoder scratch the caller owns: given, or a grow-only device buffer kept by this wrapper (one call in
        flight at a time, as the tests and benchmarks use it)."""
        if d_scratch is not None:
            return d_scratch
        import torch
        cur = getattr(self, "_dec_scratch", None)
        if cur is None or cur.numel() < nbytes:
            torch.cuda.synchronize()
            self._dec_scratch = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
        return self._dec_scratch

    def pusch_decode_batch(self, cfg, n_tb, d_llr, llr_stride, d_soft, d_state, d_tb, tb_stride, d_result, stream=None,
                           d_scratch=None):
        """pusch_decoder for n_tb transport blocks of one configuration, everything resident in HBM."""
        scratch = C.c_uint64(0)
        _check(self.lib.nrphy_pusch_decoder_sizes(self.handle, C.byref(cfg), n_tb, None, None, C.byref(scratch), None),
               "nrphy_pusch_decoder_sizes")
        d_scratch = self._scratch(scratch.value, d_scratch)
        _check(self.lib.nrphy_pusch_decode_batch(self.handle, C.byref(cfg), n_tb, _dptr(d_llr), llr_stride, _dptr(d_soft),
                                                 _dptr(d_state), _dptr(d_scratch), _dptr(d_tb), tb_stride, _dptr(d_result),
                                                 _stream(stream)), "nrphy_pusch_decode_batch")

    def ldpc_decoder_scratch_bytes(self, cfg, n_cb):
        b = C.c_uint64(0)
        _check(self.lib.nrphy_ldpc_decoder_scratch_bytes(self.handle, C.byref(cfg), n_cb, C.byref(b)),
               "nrphy_ldpc_decoder_scratch_bytes")
        return int(b.value)

    def ldpc_decode(self, cfg, n_cb, d_llr, llr_stride, d_out, out_stride, d_iterations=None, stream=None, d_scratch=None):
        """ldpc_decoder::decode for n_cb codeblocks resident in HBM (cfg: abi.LdpcDecoderCfg)."""
        d_scratch = self._scratch(self.ldpc_decoder_scratch_bytes(cfg, max(1, n_cb)), d_scratch)
        _check(self.lib.nrphy_ldpc_decode(self.handle, C.byref(cfg), n_cb, _dptr(d_llr), llr_stride, _dptr(d_out),
                                          out_stride, _dptr(d_iterations) if d_iterations is not None else None,
                                          _dptr(d_scratch), _stream(stream)), "nrphy_ldpc_decode")

    def ldpc_decode_host(self, base_graph, lifting_size, nof_filler, crc_poly, max_iterations, scaling, llr):
        """ldpc_decoder::decode on host spans: returns (iterations or 0, Kb*Zc hard bits one per byte)."""
        llr = np.ascontiguousarray(llr, dtype=np.int8)
        cfg = abi.LdpcDecoderCfg(base_graph, lifting_size, nof_filler, crc_poly, llr.size, max_iterations, scaling)
        k = (22 if base_graph == 1 else 10) * lifting_size
        packed = np.zeros((k + 7) // 8, np.uint8)
        it = C.c_uint32(0)
        _check(self.lib.nrphy_ldpc_decode_host(self.handle, C.byref(cfg), llr.ctypes.data, packed.ctypes.data,
                                               C.byref(it)), "nrphy_ldpc_decode_host")
        return int(it.value), np.unpackbits(packed)[:k]

    def channel_equalize(self, algorithm, n_batch, nof_re, nof_layers, nof_rx_ports, d_rx, d_ch, d_noise_vars, tx_scaling, d_eq,
                         d_eq_nvars, stream=None):
        """channel_equalizer::equalize for n_batch problems in device memory: d_rx [batch][port][re] cbf16, d_ch
        [batch][layer][port][re] cbf16, d_noise_vars [batch][port] f32 -> d_eq [batch][re][layer] complex64, d_eq_nvars f32."""
        _check(self.lib.nrphy_channel_equalize(self.handle, algorithm, n_batch, nof_re, nof_layers, nof_rx_ports, _dptr(d_rx),
                                               _dptr(d_ch), _dptr(d_noise_vars), tx_scaling, _dptr(d_eq), _dptr(d_eq_nvars),
                                               _stream(stream)), "nrphy_channel_equalize")

    def channel_equalize_host(self, algorithm, rx, ch, noise_vars, tx_scaling=1.0):
        """One problem from host memory: rx [port][re] and ch [layer][port][re] as raw cbf16 words (uint32) ->
        (symbols complex64 [re][layer], noise variances float32 [re][layer])."""
        rx = np.ascontiguousarray(rx, dtype=np.uint32)
        ch = np.ascontiguousarray(ch, dtype=np.uint32)
        noise_vars = np.ascontiguousarray(noise_vars, dtype=np.float32)
        nof_layers, nof_ports, nof_re = ch.shape
        eq = np.zeros((nof_re, nof_layers), np.complex64)
        nv = np.zeros((nof_re, nof_layers), np.float32)
        _check(self.lib.nrphy_channel_equalize_host(self.handle, algorithm, nof_re, nof_layers, nof_ports, rx.ctypes.data,
                                                    ch.ctypes.data, noise_vars.ctypes.data, tx_scaling, eq.ctypes.data,
                                                    nv.ctypes.data), "nrphy_channel_equalize_host")
        return eq, nv

    def pusch_demodulate_host(self, cfg, grid, ch_est, noise_vars):
        """pusch_demodulator::demodulate for one PUSCH: grid [ports][14][subc] and ch_est [layers][rx][14][subc] as raw cbf16
        words (uint32), noise_vars [rx] -> (descrambled int8 soft bits, SINR in dB)."""
        grid = np.ascontiguousarray(grid, dtype=np.uint32)
        ch_est = np.ascontiguousarray(ch_est, dtype=np.uint32)
        nv = np.ascontiguousarray(noise_vars, dtype=np.float32)
        out = np.zeros(pusch_demod_codeword_bits(cfg), np.int8)
        sinr = C.c_float(0)
        _check(self.lib.nrphy_pusch_demodulate_host(self.handle, C.byref(cfg), grid.ctypes.data, grid.shape[0], grid.shape[-1],
                                                    ch_est.ctypes.data, nv.ctypes.data, out.ctypes.data, C.byref(sinr)),
               "nrphy_pusch_demodulate_host")
        return out, float(sinr.value)

    def pusch_demodulate_host_ex(self, cfg, grid, ch_est, noise_vars, features):
        """pusch_demodulate_host with a feature mask (abi.PUSCH_DEMOD_*): transform precoding and pi/2-BPSK."""
        grid = np.ascontiguousarray(grid, dtype=np.uint32)
        ch_est = np.ascontiguousarray(ch_est, dtype=np.uint32)
        nv = np.ascontiguousarray(noise_vars, dtype=np.float32)
        out = np.zeros(pusch_demod_codeword_bits(cfg), np.int8)
        sinr = C.c_float(0)
        _check(self.lib.nrphy_pusch_demodulate_host_ex(self.handle, C.byref(cfg), grid.ctypes.data, grid.shape[0], grid.shape[-1],
                                                       ch_est.ctypes.data, nv.ctypes.data, features, out.ctypes.data,
                                                       C.byref(sinr)), "nrphy_pusch_demodulate_host_ex")
        return out, float(sinr.value)

    def pusch_demodulate_host_evm(self, cfg, grid, ch_est, noise_vars, features=0):
        """pusch_demodulate_host_ex with the EVM of the reference's evm_calculator: (soft bits, SINR in dB, EVM as np.float32)."""
        grid = np.ascontiguousarray(grid, dtype=np.uint32)
        ch_est = np.ascontiguousarray(ch_est, dtype=np.uint32)
        nv = np.ascontiguousarray(noise_vars, dtype=np.float32)
        out = np.zeros(pusch_demod_codeword_bits(cfg), np.int8)
        sinr, evm = C.c_float(0), C.c_float(0)
        _check(self.lib.nrphy_pusch_demodulate_host_evm(self.handle, C.byref(cfg), grid.ctypes.data, grid.shape[0], grid.shape[-1],
                                                        ch_est.ctypes.data, nv.ctypes.data, features, out.ctypes.data,
                                                        C.byref(sinr), C.byref(evm)), "nrphy_pusch_demodulate_host_evm")
        return out, float(sinr.value), np.float32(evm.value)

    def pusch_chest_host(self, cfg, grid, ch_est=None, lowpapr=None, ex=False):
        """dmrs_pusch_estimator::estimate + the processor's DC step for one PUSCH: grid [ports][14][subc] raw cbf16 words ->
        (ch_est [layers][rx][14][subc] cbf16 words, noise_vars [rx], measurements [rx][2] of abi.PuschChestMeas).  ch_est: the
        buffer to write into (only the allocated region changes); zeros when None.  lowpapr: an abi.PuschChestLowpapr for
        nrphy_pusch_chest_host_ex; ex = True calls that form with whatever lowpapr is (None: a null pointer)."""
        grid = np.ascontiguousarray(grid, dtype=np.uint32)
        shape = (cfg.nof_tx_layers, cfg.nof_rx_ports, 14, grid.shape[-1])
        ce = np.zeros(shape, np.uint32) if ch_est is None else np.array(ch_est, dtype=np.uint32, order="C")
        if ce.shape != shape:
            raise ValueError("ch_est must be %s" % (shape,))
        nv = np.zeros(cfg.nof_rx_ports, np.float32)
        meas = (abi.PuschChestMeas * (cfg.nof_rx_ports * abi.PUSCH_CHEST_MAX_LAYERS))()
        if ex or lowpapr is not None:
            _check(self.lib.nrphy_pusch_chest_host_ex(self.handle, C.byref(cfg), None if lowpapr is None else C.byref(lowpapr),
                                                      grid.ctypes.data, grid.shape[0], grid.shape[-1], ce.ctypes.data, nv.ctypes.data,
                                                      meas), "nrphy_pusch_chest_host_ex")
        else:
            _check(self.lib.nrphy_pusch_chest_host(self.handle, C.byref(cfg), grid.ctypes.data, grid.shape[0], grid.shape[-1],
                                                   ce.ctypes.data, nv.ctypes.data, meas), "nrphy_pusch_chest_host")
        m = [[meas[i * abi.PUSCH_CHEST_MAX_LAYERS + l] for l in range(abi.PUSCH_CHEST_MAX_LAYERS)] for i in range(cfg.nof_rx_ports)]
        return ce, nv, m

    def pusch_lowpapr_sequence_host(self, n_rs_id, nof_prb):
        """The low-PAPR DM-RS of a transform-precoded PUSCH from the kernel's generator: complex64 [6 nof_prb]
        (nrphy_pusch_lowpapr_sequence_host)."""
        out = np.zeros(6 * nof_prb, np.complex64)
        _check(self.lib.nrphy_pusch_lowpapr_sequence_host(self.handle, n_rs_id, nof_prb, out.ctypes.data),
               "nrphy_pusch_lowpapr_sequence_host")
        return out

    def pusch_tp_host(self, pdu, tp, options, grid, harq_soft=None, harq_state=None):
        """pusch_proc_host with an abi.PuschTpDesc (or None: a null pointer) and an abi.PuschEvmOptions (nrphy_pusch_tp_host)."""
        grid = np.ascontiguousarray(grid, dtype=np.uint32)
        soft_bytes, state_bytes = pusch_tp_harq_bytes(pdu, tp, options)
        soft = np.zeros(soft_bytes, np.int8) if harq_soft is None else harq_soft
        state = np.zeros(state_bytes, np.uint8) if harq_state is None else harq_state
        if soft.size != soft_bytes or state.size != state_bytes or not (soft.flags.c_contiguous and state.flags.c_contiguous):
            raise ValueError("HARQ blocks must be contiguous arrays of %d and %d bytes" % (soft_bytes, state_bytes))
        tb = np.zeros(pdu.tb_size_bytes, np.uint8)
        uci = np.zeros(pdu.nof_harq_ack + pdu.nof_csi_part1, np.uint8)
        result = abi.PuschResult()
        _check(self.lib.nrphy_pusch_tp_host(self.handle, C.byref(pdu), None if tp is None else C.byref(tp), C.byref(options),
                                            grid.ctypes.data, grid.shape[0], grid.shape[-1], soft.ctypes.data if soft_bytes else None,
                                            state.ctypes.data if state_bytes else None, tb.ctypes.data if tb.size else None,
                                            uci.ctypes.data if uci.size else None, C.byref(result)), "nrphy_pusch_tp_host")
        return result, tb, uci

    def pusch_evm_host(self, pdu, options, grid, harq_soft=None, harq_state=None):
        """pusch_proc_host with abi.PuschEvmOptions (nrphy_pusch_evm_host): with enable_evm the result carries the EVM."""
        return self.pusch_proc_host(pdu, options, grid, harq_soft, harq_state)

    def pusch_proc_host(self, pdu, options, grid, harq_soft=None, harq_state=None):
        """pusch_processor::process for one PDU: grid [ports][14][subc] raw cbf16 words -> (abi.PuschResult, transport block bytes,
        UCI payload bits: HARQ-ACK then CSI part 1, one per byte).  harq_soft / harq_state: the PDU's HARQ blocks (int8 / uint8
        arrays of pusch_proc_harq_bytes(pdu, options)), read and written in place; fresh zeroed ones when None.  options: an
        abi.PuschProcOptions, or an abi.PuschEvmOptions for nrphy_pusch_evm_host."""
        grid = np.ascontiguousarray(grid, dtype=np.uint32)
        with_evm = isinstance(options, abi.PuschEvmOptions)
        call = self.lib.nrphy_pusch_evm_host if with_evm else self.lib.nrphy_pusch_proc_host
        sizing = options
        if with_evm:  # the HARQ sizes do not depend on the SINR method, and nrphy_pusch_proc_harq_bytes refuses the EVM-based one
            sizing = abi.PuschProcOptions(options.proc.dec_nof_iterations, options.proc.dec_enable_early_stop,
                                          abi.PUSCH_SINR_CHANNEL_ESTIMATOR, options.proc.equalizer)
        soft_bytes, state_bytes = pusch_proc_harq_bytes(pdu, sizing)
        soft = np.zeros(soft_bytes, np.int8) if harq_soft is None else harq_soft
        state = np.zeros(state_bytes, np.uint8) if harq_state is None else harq_state
        if soft.size != soft_bytes or state.size != state_bytes or not (soft.flags.c_contiguous and state.flags.c_contiguous):
            raise ValueError("HARQ blocks must be contiguous arrays of %d and %d bytes" % (soft_bytes, state_bytes))
        tb = np.zeros(pdu.tb_size_bytes, np.uint8)
        uci = np.zeros(pdu.nof_harq_ack + pdu.nof_csi_part1, np.uint8)
        result = abi.PuschResult()
        _check(call(self.handle, C.byref(pdu), C.byref(options), grid.ctypes.data, grid.shape[0],
                    grid.shape[-1], soft.ctypes.data if soft_bytes else None,
                    state.ctypes.data if state_bytes else None, tb.ctypes.data if tb.size else None,
                    uci.ctypes.data if uci.size else None, C.byref(result)),
               "nrphy_pusch_evm_host" if with_evm else "nrphy_pusch_proc_host")
        return result, tb, uci

    def pusch_csi2_host(self, pdu, desc, options, grid, harq_soft=None, harq_state=None, csi2_fill=0):
        """pusch_processor::process for one PDU with a CSI part 2 description: as pusch_proc_host, and returns (abi.PuschResult,
        abi.PuschCsi2Result, transport block bytes, UCI payload bits, CSI part 2 bits).  The part 2 array has room for the largest
        size of the description and starts filled with csi2_fill; the first nof_csi_part2 bytes are the payload."""
        grid = np.ascontiguousarray(grid, dtype=np.uint32)
        soft_bytes, state_bytes = pusch_csi2_harq_bytes(pdu, desc, options)
        soft = np.zeros(soft_bytes, np.int8) if harq_soft is None else harq_soft
        state = np.zeros(state_bytes, np.uint8) if harq_state is None else harq_state
        if soft.size != soft_bytes or state.size != state_bytes or not (soft.flags.c_contiguous and state.flags.c_contiguous):
            raise ValueError("HARQ blocks must be contiguous arrays of %d and %d bytes" % (soft_bytes, state_bytes))
        table = pusch_csi2_variants(pdu, desc, options, grid.shape[0], grid.shape[-1])
        if table is None:
            raise ValueError("nrphy_pusch_csi2_validate refuses the PDU")
        tb = np.zeros(pdu.tb_size_bytes, np.uint8)
        uci = np.zeros(pdu.nof_harq_ack + pdu.nof_csi_part1, np.uint8)
        csi2 = np.full(table[0][-1], csi2_fill, np.uint8)
        result, csi2_result = abi.PuschResult(), abi.PuschCsi2Result()
        _check(self.lib.nrphy_pusch_csi2_host(self.handle, C.byref(pdu), C.byref(desc), C.byref(options), grid.ctypes.data,
                                              grid.shape[0], grid.shape[-1], soft.ctypes.data if soft_bytes else None,
                                              state.ctypes.data if state_bytes else None, tb.ctypes.data if tb.size else None,
                                              uci.ctypes.data if uci.size else None, csi2.ctypes.data if csi2.size else None,
                                              C.byref(result), C.byref(csi2_result)), "nrphy_pusch_csi2_host")
        return result, csi2_result, tb, uci, csi2

    def prach_detect_host(self, cfg, symbols, with_metric=False):
        """prach_detector::detect for one occasion: symbols [ports][symbols][L_RA] complex64 -> (abi.PrachResult, the 64
        abi.PrachPreamble slots, and with_metric the metric windows [64][window width] f32 or None)."""
        symbols = np.ascontiguousarray(symbols, dtype=np.complex64)
        if symbols.ndim != 3 or symbols.shape[0] < cfg.nof_rx_ports:
            raise ValueError("symbols must be [ports][symbols][L_RA]")
        width = int(self.lib.nrphy_prach_window_width(C.byref(cfg)))
        result = abi.PrachResult()
        pre = (abi.PrachPreamble * abi.PRACH_MAX_PREAMBLES)()
        metric = np.zeros((abi.PRACH_MAX_PREAMBLES, width), np.float32) if with_metric else None
        _check(self.lib.nrphy_prach_detect_host(self.handle, C.byref(cfg), symbols.ctypes.data, symbols.shape[1] * symbols.shape[2],
                                                symbols.shape[2], C.byref(result), pre,
                                                metric.ctypes.data if with_metric else None), "nrphy_prach_detect_host")
        return result, pre, metric

    def prach_generate_host(self, cfg, preamble_index):
        """prach_generator::generate: the frequency-domain sequence of one preamble, L_RA complex64."""
        y = np.zeros(839 if cfg.format < 4 else 139, np.complex64)
        _check(self.lib.nrphy_prach_generate_host(self.handle, C.byref(cfg), preamble_index, y.ctypes.data), "nrphy_prach_generate_host")
        return y

    def prach_demodulate_host(self, cfg, samples, symbols=None):
        """ofdm_prach_demodulator::demodulate for every port of one configuration: samples [ports][>= window_samples] complex64 ->
        symbols [ports][td][fd][symbols][L_RA] complex64 (the prach_buffer's order).  symbols: a larger C-contiguous buffer of five
        dimensions to write into (only the configuration's elements change); zeros of the exact size when None."""
        samples = np.ascontiguousarray(samples, dtype=np.complex64)
        sz = prach_demod_sizes(cfg)
        if sz is None:
            raise ValueError("nrphy_prach_demod_validate refuses the configuration")
        if samples.ndim != 2 or samples.shape[0] < cfg.nof_rx_ports or samples.shape[1] < sz.window_samples:
            raise ValueError("samples must be [ports][>= %d]" % sz.window_samples)
        shape = (cfg.nof_rx_ports, cfg.nof_td_occasions, cfg.nof_fd_occasions, sz.nof_symbols, sz.sequence_length)
        out = np.zeros(shape, np.complex64) if symbols is None else np.array(symbols, dtype=np.complex64, order="C")
        if out.ndim != 5 or any(a < b for a, b in zip(out.shape, shape)):
            raise ValueError("symbols must be at least %s" % (shape,))
        st = [v // 8 for v in out.strides]  # port, td, fd, symbol, re
        _check(self.lib.nrphy_prach_demodulate_host(self.handle, C.byref(cfg), samples.ctypes.data, samples.shape[1], out.ctypes.data,
                                                    st[0], st[2], st[1], st[3]), "nrphy_prach_demodulate_host")
        return out

    def pucch_host(self, cfg, grid, with_estimate=False, ch_est=None):
        """pucch_processor::process (format 0 or 1) for one PUCCH: grid [ports][14][subc] raw cbf16 words -> (abi.PucchResult,
        measurements [rx] of abi.PuschChestMeas, and with_estimate format 1's ch_est [rx][14][subc] cbf16 words or None).  ch_est:
        the buffer to write into (only the allocated region changes); zeros when None."""
        grid = np.ascontiguousarray(grid, dtype=np.uint32)
        result = abi.PucchResult()
        meas = (abi.PuschChestMeas * cfg.nof_rx_ports)()
        ce = None
        if with_estimate:
            shape = (cfg.nof_rx_ports, 14, grid.shape[-1])
            ce = np.zeros(shape, np.uint32) if ch_est is None else np.array(ch_est, dtype=np.uint32, order="C")
            if ce.shape != shape:
                raise ValueError("ch_est must be %s" % (shape,))
        _check(self.lib.nrphy_pucch_host(self.handle, C.byref(cfg), grid.ctypes.data, grid.shape[0], grid.shape[-1], C.byref(result),
                                         meas, ce.ctypes.data if with_estimate else None), "nrphy_pucch_host")
        return result, list(meas), ce

    def pf2_host(self, cfg, grid, with_estimate=False, ch_est=None, fill=0):
        """pucch_processor::process (format 2) for one PUCCH: grid [ports][14][subc] raw cbf16 words -> dict of message uint8 [A]
        (one bit per byte; bytes the decoder does not write hold `fill`), status, csi (abi.Pf2Csi), meas [rx] of abi.PuschChestMeas,
        llr int8 [E] and, with_estimate, ch_est [rx][14][subc] cbf16 words (else None).  ch_est: the buffer to write into (only the
        allocation changes); zeros when None."""
        grid = np.ascontiguousarray(grid, dtype=np.uint32)
        sizes = pf2_sizes(cfg)
        if sizes is None:
            raise ValueError("nrphy_pf2_validate refuses the configuration")
        E, A = sizes
        message = np.full(A, fill, np.uint8)
        llr = np.zeros(E, np.int8)
        status = C.c_uint32()
        csi = abi.Pf2Csi()
        meas = (abi.PuschChestMeas * cfg.nof_rx_ports)()
        ce = None
        if with_estimate:
            shape = (cfg.nof_rx_ports, 14, grid.shape[-1])
            ce = np.zeros(shape, np.uint32) if ch_est is None else np.array(ch_est, dtype=np.uint32, order="C")
            if ce.shape != shape:
                raise ValueError("ch_est must be %s" % (shape,))
        _check(self.lib.nrphy_pf2_host(self.handle, C.byref(cfg), grid.ctypes.data, grid.shape[0], grid.shape[-1], message.ctypes.data,
                                       C.byref(status), C.byref(csi), meas, ce.ctypes.data if with_estimate else None,
                                       llr.ctypes.data), "nrphy_pf2_host")
        return {"message": message, "status": int(status.value), "csi": csi, "meas": list(meas), "llr": llr, "ch_est": ce}

    def srs_host(self, cfg, grid):
        """srs_estimator::estimate for one SRS: grid [ports][14][subc] raw cbf16 words -> abi.SrsResult."""
        grid = np.ascontiguousarray(grid, dtype=np.uint32)
        result = abi.SrsResult()
        _check(self.lib.nrphy_srs_host(self.handle, C.byref(cfg), grid.ctypes.data, grid.shape[0], grid.shape[-1], C.byref(result)),
               "nrphy_srs_host")
        return result

    def srs_sequence_host(self, cfg, antenna_port):
        """The low-PAPR sequence of one antenna port, cyclic shift included, from the estimator's device generator: complex64 [M]."""
        info = srs_info(cfg, antenna_port)
        if info is None:
            raise ValueError("nrphy_srs_info refuses the configuration")
        out = np.zeros(info["sequence_length"], np.complex64)
        _check(self.lib.nrphy_srs_sequence_host(self.handle, C.byref(cfg), antenna_port, out.ctypes.data), "nrphy_srs_sequence_host")
        return out

    def uci_decode_host(self, cfg, llr, fill=0):
        """uci_decoder::decode for one message: llr int8 [llr_length] -> (message uint8 [message_length], one bit per byte, status).
        Bytes the decoder does not write (a second block behind a failed first one) hold `fill`."""
        llr = np.ascontiguousarray(llr, dtype=np.int8)
        if llr.size != cfg.llr_length:
            raise ValueError("llr must hold %d soft bits" % cfg.llr_length)
        message = np.full(cfg.message_length, fill, np.uint8)
        status = C.c_uint32()
        _check(self.lib.nrphy_uci_decode_host(self.handle, C.byref(cfg), llr.ctypes.data, message.ctypes.data, C.byref(status)),
               "nrphy_uci_decode_host")
        return message, int(status.value)

    def ulsch_demultiplex_host(self, cfg, codeword_llr, fill=0):
        """ulsch_demultiplex for one codeword: int8 [nof_codeword_bits] -> (sch, harq_ack, csi1, csi2) int8 arrays of
        nof_sch_bits and the configuration's nof_enc_* bits, allocated holding `fill`."""
        sizes = ulsch_demux_sizes(cfg)
        if sizes is None:
            raise NrphyError(abi.ERR_ARGUMENT, "nrphy_ulsch_demux_sizes")
        llr = np.ascontiguousarray(codeword_llr, dtype=np.int8)
        if llr.size != sizes[1]:
            raise ValueError("the codeword must hold %d soft bits" % sizes[1])
        out = [np.full(n, fill, np.int8) for n in (sizes[0], cfg.nof_enc_harq_ack_bits, cfg.nof_enc_csi_part1_bits,
                                                   cfg.nof_enc_csi_part2_bits)]
        _check(self.lib.nrphy_ulsch_demultiplex_host(self.handle, C.byref(cfg), llr.ctypes.data, *[o.ctypes.data if o.size else None
                                                                                                  for o in out]),
               "nrphy_ulsch_demultiplex_host")
        return tuple(out)

    def dft(self, size, inverse, batch, d_in, d_out, stream=None):
        _check(self.lib.nrphy_dft_run(self.handle, size, int(inverse), batch, _dptr(d_in), _dptr(d_out), _stream(stream)),
               "nrphy_dft_run")

    def transform_deprecode(self, nof_prb, batch, d_in, d_out, stream=None):
        """transform_precoder::deprecode_ofdm_symbol for `batch` symbols of 12 * nof_prb complex64 in device memory; d_out may be
        d_in."""
        _check(self.lib.nrphy_transform_deprecode(self.handle, nof_prb, batch, _dptr(d_in), _dptr(d_out), _stream(stream)),
               "nrphy_transform_deprecode")

    def transform_deprecode_host(self, nof_prb, symbols):
        """One symbol of 12 * nof_prb complex64 from host memory -> the deprecoded symbol."""
        x = np.ascontiguousarray(symbols, dtype=np.complex64)
        if x.shape != (12 * nof_prb,):
            raise ValueError("a symbol of %d PRB has %d elements" % (nof_prb, 12 * nof_prb))
        out = np.zeros_like(x)
        _check(self.lib.nrphy_transform_deprecode_host(self.handle, nof_prb, x.ctypes.data, out.ctypes.data),
               "nrphy_transform_deprecode_host")
        return out


class PdschPlan:
    """nrphy_pdsch_plan: a batch of PDUs with their grids; run() launches the whole PDSCH path."""

    def __init__(self, ctx, pdus, tb_offsets, grid_indices, nof_grids, nof_ports, nof_subc):
        self.ctx = ctx
        n = len(pdus)
        arr = (abi.PdschPdu * n)(*pdus)
        self._keep = [getattr(p, "_keepalive", None) for p in pdus]
        offs = (C.c_uint64 * n)(*tb_offsets)
        gidx = (C.c_uint32 * n)(*grid_indices)
        h = C.c_void_p()
        _check(ctx.lib.nrphy_pdsch_plan_create(ctx.handle, n, arr, offs, gidx, nof_grids, nof_ports, nof_subc,
                                               C.byref(h)), "nrphy_pdsch_plan_create")
        self.handle = h
        self.nof_grids, self.nof_ports, self.nof_subc = nof_grids, nof_ports, nof_subc

    @property
    def nof_codeblocks(self):
        return int(self.ctx.lib.nrphy_pdsch_plan_nof_codeblocks(self.handle))

    @property
    def codeword_bits(self):
        return int(self.ctx.lib.nrphy_pdsch_plan_codeword_bits(self.handle))

    def codeword_offset(self, pdu):
        return int(self.ctx.lib.nrphy_pdsch_plan_codeword_offset(self.handle, pdu))

    @property
    def nof_sequences(self):
        """(distinct scrambling sequences, distinct DM-RS sequence sets) a run of the plan generates."""
        scr, dmrs = C.c_uint32(0), C.c_uint32(0)
        _check(self.ctx.lib.nrphy_pdsch_plan_nof_sequences(self.handle, C.byref(scr), C.byref(dmrs)), "nrphy_pdsch_plan_nof_sequences")
        return int(scr.value), int(dmrs.value)

    @property
    def scrambling_form(self):
        """"words" or "seeds": how a run hands the distinct scrambling sequences to the codeblock waves."""
        form = int(self.ctx.lib.nrphy_pdsch_plan_scrambling_form(self.handle))
        if form < 0:
            raise NrphyError(abi.ERR_ARGUMENT, "nrphy_pdsch_plan_scrambling_form")
        return "words" if form else "seeds"

    @property
    def codeblock_dispatch(self):
        """"mixed" or "bucket": one launch of the mixed codeblock kernel, or one launch per (Qm, layers) bucket."""
        dispatch = int(self.ctx.lib.nrphy_pdsch_plan_codeblock_dispatch(self.handle))
        if dispatch < 0:
            raise NrphyError(abi.ERR_ARGUMENT, "nrphy_pdsch_plan_codeblock_dispatch")
        return "mixed" if dispatch == 1 else "bucket"

    def run(self, d_tb, d_grid, d_cw_rm=None, d_cw_scr=None, zero_grids=True, stream=None):
        _check(self.ctx.lib.nrphy_pdsch_run(self.handle, _dptr(d_tb), _dptr(d_grid), _dptr(d_cw_rm), _dptr(d_cw_scr),
                                            int(zero_grids), _stream(stream)), "nrphy_pdsch_run")

    def enable_timing(self, max_runs, stride=1):
        """Records HIP events around the kernels of the next runs: every `stride`-th one, up to max_runs of them."""
        _check(self.ctx.lib.nrphy_pdsch_plan_enable_timing(self.handle, max_runs), "nrphy_pdsch_plan_enable_timing")
        _check(self.ctx.lib.nrphy_pdsch_plan_timing_stride(self.handle, stride), "nrphy_pdsch_plan_timing_stride")

    def kernel_times(self):
        """Average ms of (tb_crc, codeblock, dmrs, whole run) over the recorded runs, and the run count."""
        ms = (C.c_float * 4)()
        n = C.c_uint32(0)
        _check(self.ctx.lib.nrphy_pdsch_plan_kernel_times(self.handle, ms, C.byref(n)), "nrphy_pdsch_plan_kernel_times")
        return [float(x) for x in ms], int(n.value)

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_pdsch_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PuschDemodPlan:
    """nrphy_pusch_demod_plan: PUSCHs over a batch of received grids; run() equalises, demaps and descrambles them in one launch."""

    def __init__(self, ctx, cfgs, grid_indices, nof_grids, nof_ports, nof_subc, ce_offsets, features=0):
        """features: abi.PUSCH_DEMOD_* bits (transform precoding, pi/2-BPSK); 0 is nrphy_pusch_demod_plan_create."""
        self.ctx = ctx
        n = len(cfgs)
        arr = (abi.PuschDemodCfg * n)(*cfgs)
        gidx = (C.c_uint32 * n)(*grid_indices)
        offs = (C.c_uint64 * n)(*ce_offsets)
        h = C.c_void_p()
        _check(ctx.lib.nrphy_pusch_demod_plan_create_ex(ctx.handle, n, arr, gidx, nof_grids, nof_ports, nof_subc, offs, features,
                                                        C.byref(h)), "nrphy_pusch_demod_plan_create_ex")
        self.handle = h
        self.n = n

    def codeword_bits(self, i):
        return int(self.ctx.lib.nrphy_pusch_demod_plan_codeword_bits(self.handle, i))

    def run(self, d_grid, d_ch_est, d_noise_vars, d_llr, llr_stride, d_sinr=None, stream=None, d_evm=None):
        """d_evm: [n] float32 for the EVM per PUSCH (nrphy_pusch_demod_run_evm); None is nrphy_pusch_demod_run."""
        if d_evm is not None:
            _check(self.ctx.lib.nrphy_pusch_demod_run_evm(self.handle, _dptr(d_grid), _dptr(d_ch_est), _dptr(d_noise_vars),
                                                          _dptr(d_llr), llr_stride, _dptr(d_sinr), _dptr(d_evm), _stream(stream)),
                   "nrphy_pusch_demod_run_evm")
            return
        _check(self.ctx.lib.nrphy_pusch_demod_run(self.handle, _dptr(d_grid), _dptr(d_ch_est), _dptr(d_noise_vars), _dptr(d_llr),
                                                  llr_stride, _dptr(d_sinr), _stream(stream)), "nrphy_pusch_demod_run")

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_pusch_demod_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PuschChestPlan:
    """nrphy_pusch_chest_plan: PUSCHs over a batch of received grids; run() writes their channel estimates (the layout
    PuschDemodPlan reads), the noise variances PuschDemodPlan.run takes and, optionally, the measurements."""

    def __init__(self, ctx, cfgs, grid_indices, nof_grids, nof_ports, nof_subc, ce_offsets, lowpapr=None, ex=False):
        """lowpapr: one abi.PuschChestLowpapr per PUSCH for nrphy_pusch_chest_plan_create_ex; ex = True calls that form with
        whatever lowpapr is (None: a null pointer)."""
        self.ctx = ctx
        n = len(cfgs)
        arr = (abi.PuschChestCfg * n)(*cfgs)
        gidx = (C.c_uint32 * n)(*grid_indices)
        offs = (C.c_uint64 * n)(*ce_offsets)
        h = C.c_void_p()
        if ex or lowpapr is not None:
            lps = None if lowpapr is None else (abi.PuschChestLowpapr * n)(*lowpapr)
            _check(ctx.lib.nrphy_pusch_chest_plan_create_ex(ctx.handle, n, arr, lps, gidx, nof_grids, nof_ports, nof_subc, offs,
                                                            C.byref(h)), "nrphy_pusch_chest_plan_create_ex")
        else:
            _check(ctx.lib.nrphy_pusch_chest_plan_create(ctx.handle, n, arr, gidx, nof_grids, nof_ports, nof_subc, offs, C.byref(h)),
                   "nrphy_pusch_chest_plan_create")
        self.handle = h
        self.n = n

    def run(self, d_grid, d_ch_est, d_noise_vars, d_meas=None, stream=None):
        """d_noise_vars: [n][4] f32; d_meas: [n][4][2] x 32 bytes (abi.PuschChestMeas) or None."""
        _check(self.ctx.lib.nrphy_pusch_chest_run(self.handle, _dptr(d_grid), _dptr(d_ch_est), _dptr(d_noise_vars), _dptr(d_meas),
                                                  _stream(stream)), "nrphy_pusch_chest_run")

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_pusch_chest_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OfhRx:
    """nrphy_ofh_rx: the uplink frame receiver of one stream of frames; it owns the sequence checker's state on the device."""

    def __init__(self, ctx, cfg):
        self.ctx = ctx
        h = C.c_void_p()
        _check(ctx.lib.nrphy_ofh_rx_create(ctx.handle, C.byref(cfg), C.byref(h)), "nrphy_ofh_rx_create")
        self.handle = h

    def run(self, frames, expects, d_frames, d_grid, nof_grids, grid_nof_ports, grid_nof_subc, d_records, frames_bytes=None, stream=None):
        """frames: a list of abi.OfhRxFrame; expects: a list of abi.OfhRxExpect; d_frames: a uint8 tensor; d_records: device memory
        for len(frames) abi.OfhRxRecord; returns the status (NRPHY_OK or NRPHY_ERR_ARGUMENT)."""
        f_arr = (abi.OfhRxFrame * max(len(frames), 1))(*frames)
        e_arr = (abi.OfhRxExpect * max(len(expects), 1))(*expects)
        frames_bytes = d_frames.numel() * d_frames.element_size() if frames_bytes is None else frames_bytes
        return int(self.ctx.lib.nrphy_ofh_rx_run(self.handle, len(frames), f_arr, len(expects), e_arr, _dptr(d_frames), frames_bytes,
                                                 _dptr(d_grid), nof_grids, grid_nof_ports, grid_nof_subc, _dptr(d_records), _stream(stream)))

    def host(self, frame, expects, grid):
        """frame: uint8 array; grid: uint32 [ports][14][subc], written in place; returns (status, abi.OfhRxRecord)."""
        frame = np.ascontiguousarray(frame, np.uint8)
        assert grid.dtype == np.uint32 and grid.flags.c_contiguous and grid.ndim == 3 and grid.shape[1] == 14
        e_arr = (abi.OfhRxExpect * max(len(expects), 1))(*expects)
        rec = abi.OfhRxRecord()
        rc = int(self.ctx.lib.nrphy_ofh_rx_host(self.handle, frame.ctypes.data, frame.size, len(expects), e_arr, grid.ctypes.data,
                                                grid.shape[0], grid.shape[2], C.byref(rec)))
        return rc, rec

    def reset(self, stream=None):
        _check(self.ctx.lib.nrphy_ofh_rx_reset(self.handle, _stream(stream)), "nrphy_ofh_rx_reset")

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_ofh_rx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PrachPlan:
    """nrphy_prach_plan: occasions of one buffer of complex64 samples; occasion i reads element sym_offsets[i] + port *
    port_stride + symbol * symbol_stride + k.  run() writes [n] abi.PrachResult, [n][64] abi.PrachPreamble and, optionally,
    [n][64][metric_stride] f32."""

    def __init__(self, ctx, cfgs, sym_offsets, port_stride, symbol_stride):
        self.ctx = ctx
        n = len(cfgs)
        arr = (abi.PrachCfg * n)(*cfgs)
        offs = (C.c_uint64 * n)(*sym_offsets)
        h = C.c_void_p()
        _check(ctx.lib.nrphy_prach_plan_create(ctx.handle, n, arr, offs, port_stride, symbol_stride, C.byref(h)),
               "nrphy_prach_plan_create")
        self.handle = h
        self.n = n
        self.metric_stride = int(ctx.lib.nrphy_prach_plan_metric_stride(h))

    def run(self, d_symbols, d_result, d_preambles, d_metric=None, stream=None):
        _check(self.ctx.lib.nrphy_prach_run(self.handle, _dptr(d_symbols), _dptr(d_result), _dptr(d_preambles), _dptr(d_metric),
                                            _stream(stream)), "nrphy_prach_run")

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_prach_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PucchPlan:
    """nrphy_pucch_plan: PUCCHs of formats 0 and 1 over a batch of received grids (the grid buffer PuschChestPlan reads); run()
    writes [n] abi.PucchResult and, optionally, [n][4] abi.PuschChestMeas and format 1's channel estimates (ce_offsets given)."""

    def __init__(self, ctx, cfgs, grid_indices, nof_grids, nof_ports, nof_subc, ce_offsets=None):
        self.ctx = ctx
        n = len(cfgs)
        arr = (abi.PucchCfg * n)(*cfgs)
        gidx = (C.c_uint32 * n)(*grid_indices)
        offs = (C.c_uint64 * n)(*ce_offsets) if ce_offsets is not None else None
        h = C.c_void_p()
        _check(ctx.lib.nrphy_pucch_plan_create(ctx.handle, n, arr, gidx, nof_grids, nof_ports, nof_subc, offs, C.byref(h)),
               "nrphy_pucch_plan_create")
        self.handle = h
        self.n = n

    def run(self, d_grid, d_result, d_meas=None, d_ch_est=None, stream=None):
        """d_result: [n] x 40 bytes; d_meas: [n][4] x 32 bytes or None; d_ch_est: what ce_offsets index, or None."""
        _check(self.ctx.lib.nrphy_pucch_run(self.handle, _dptr(d_grid), _dptr(d_result), _dptr(d_meas), _dptr(d_ch_est),
                                            _stream(stream)), "nrphy_pucch_run")

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_pucch_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SrsPlan:
    """nrphy_srs_plan: sounding reference signals over a batch of received grids (the grid buffer PuschChestPlan, PucchPlan and
    Pf2Plan read); run() writes every SRS's channel matrix and time alignment with two launches."""

    def __init__(self, ctx, cfgs, grid_indices, nof_grids, nof_ports, nof_subc):
        self.ctx = ctx
        n = len(cfgs)
        arr = (abi.SrsCfg * n)(*cfgs)
        gidx = (C.c_uint32 * n)(*grid_indices)
        h = C.c_void_p()
        _check(ctx.lib.nrphy_srs_plan_create(ctx.handle, n, arr, gidx, nof_grids, nof_ports, nof_subc, C.byref(h)),
               "nrphy_srs_plan_create")
        self.handle = h
        self.n = n

    def run(self, d_grid, d_result, stream=None):
        """d_result: [n] abi.SrsResult (208 bytes each), 8-byte aligned."""
        _check(self.ctx.lib.nrphy_srs_run(self.handle, _dptr(d_grid), _dptr(d_result), _stream(stream)), "nrphy_srs_run")

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.nrphy_srs_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pf2Plan:
    """nrphy_pf2_plan: PUCCHs of format 2 over a batch of received grids (the grid buffer PuschChestPlan and PucchPlan read);
    run() writes every PUCCH's soft bits, payload bits, status and channel state information with two launches."""

    def __init__(self, ctx, cfgs, grid_indices, nof_grids, nof_ports, nof_subc, llr_offsets, message_offsets, ce_offsets=None):
        self.ctx = ctx
        n = len(cfgs)
        arr = (abi.Pf2Cfg * n)(*cfgs)
        gidx = (C.c_uint32 * n)(*grid_indices)
        lo = (C.c_uint64 * n)(*llr_offsets)
        mo = (C.c_uint64 * n)(*message_offsets)
        offs = (C.c_uint64 * n)(*ce_offsets) if ce_offsets is not None else None
        h = C.c_void_p()
        _check(ctx.lib.nrphy_pf2_plan_create(ctx.handle, n, arr, gidx, nof_grids, nof_ports, nof_subc, lo, mo, offs, C.byref(h)),
               "nrphy_pf2_plan_create")
        self.handle = h
        self.n = n

    def run(self, d_grid, d_llr, d_message, d_status, d_csi, d_meas=None, d_ch_est=None, stream=None):
        """d_llr int8, d_message uint8, d_status [n] u32 (both None: the receiver launch alone), d_csi [n] Pf2Csi; d_meas [n][4]
        PuschChestMeas or None; d_ch_est or None."""
        _check(self.ctx.lib.nrphy_pf2_run(self.handle, _dptr(d_grid), _dptr(d_llr), _dptr(d_message), _dptr(d_status), _dptr(d_csi),
                                          _dptr(d_meas), _dptr(d_ch_est), _stream(stream)), "nrphy_pf2_run")

    def close(self):
        if getattr(self, "handle", None):
            self.ctx.lib.nrphy_pf2_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class UciDecoderPlan:
    """nrphy_uci_decoder_plan: a batch of UCI messages of any sizes (short blocks and polar); run() writes every message, one
    bit per byte, and [n] uint32 statuses in one launch."""

    def __init__(self, ctx, cfgs, llr_offsets, message_offsets):
        self.ctx = ctx
        n = len(cfgs)
        arr = (abi.UciDecoderCfg * n)(*cfgs)
        lo = (C.c_uint64 * n)(*llr_offsets)
        mo = (C.c_uint64 * n)(*message_offsets)
        h = C.c_void_p()
        _check(ctx.lib.nrphy_uci_decoder_plan_create(ctx.handle, n, arr, lo, mo, C.byref(h)), "nrphy_uci_decoder_plan_create")
        self.handle = h
        self.n = n

    def run(self, d_llr, d_message, d_status, stream=None):
        """d_llr: int8 soft bits; d_message: uint8; d_status: [n] uint32 (int32 tensors do)."""
        _check(self.ctx.lib.nrphy_uci_decoder_run(self.handle, _dptr(d_llr), _dptr(d_message), _dptr(d_status), _stream(stream)),
               "nrphy_uci_decoder_run")

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_uci_decoder_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class UlschDemuxPlan:
    """nrphy_ulsch_demux_plan: a batch of PUSCH codewords with UCI; run() splits every codeword's soft bits into its UL-SCH,
    HARQ-ACK, CSI part 1 and CSI part 2 streams in one launch."""

    def __init__(self, ctx, cfgs, in_offsets, sch_offsets, harq_offsets=None, csi1_offsets=None, csi2_offsets=None):
        self.ctx = ctx
        n = len(cfgs)
        arr = (abi.UlschDemuxCfg * n)(*cfgs)
        offs = [None if o is None else (C.c_uint64 * n)(*o) for o in (in_offsets, sch_offsets, harq_offsets, csi1_offsets, csi2_offsets)]
        h = C.c_void_p()
        _check(ctx.lib.nrphy_ulsch_demux_plan_create(ctx.handle, n, arr, *offs, C.byref(h)), "nrphy_ulsch_demux_plan_create")
        self.handle = h
        self.n = n

    def run(self, d_codeword_llr, d_sch, d_harq_ack=None, d_csi1=None, d_csi2=None, stream=None):
        """int8 device buffers; a stream no codeword of the plan has may be None."""
        ptr = [None if t is None else _dptr(t) for t in (d_codeword_llr, d_sch, d_harq_ack, d_csi1, d_csi2)]
        _check(self.ctx.lib.nrphy_ulsch_demux_run(self.handle, *ptr, _stream(stream)), "nrphy_ulsch_demux_run")

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_ulsch_demux_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PuschProcPlan:
    """nrphy_pusch_proc_plan: PUSCH PDUs over a batch of received grids; run() goes from the grids to the transport blocks, the
    UCI payloads and one abi.PuschResult per PDU on one stream.  The plan owns every buffer between the stages; the caller owns
    the HARQ arena, the transport blocks, the UCI payload bytes and the results.  options: an abi.PuschProcOptions, or an
    abi.PuschEvmOptions for nrphy_pusch_evm_plan_create (the results then carry the EVM)."""

    def __init__(self, ctx, pdus, options, grid_indices, nof_grids, nof_ports, nof_subc, harq_soft_offsets=None,
                 harq_state_offsets=None, tb_offsets=None, uci_offsets=None):
        self.ctx = ctx
        n = len(pdus)
        arr = (abi.PuschPdu * n)(*pdus)
        gidx = (C.c_uint32 * n)(*grid_indices)
        offs = [None if o is None else (C.c_uint64 * n)(*o) for o in (harq_soft_offsets, harq_state_offsets, tb_offsets, uci_offsets)]
        h = C.c_void_p()
        with_evm = isinstance(options, abi.PuschEvmOptions)
        create = ctx.lib.nrphy_pusch_evm_plan_create if with_evm else ctx.lib.nrphy_pusch_proc_plan_create
        _check(create(ctx.handle, n, arr, C.byref(options), gidx, nof_grids, nof_ports, nof_subc, *offs, C.byref(h)),
               "nrphy_pusch_evm_plan_create" if with_evm else "nrphy_pusch_proc_plan_create")
        self.handle = h
        self.n = n

    def harq_bytes(self, i):
        """(soft bytes, state bytes) of PDU i's HARQ blocks; zeros without codeword."""
        soft, state = C.c_uint64(0), C.c_uint64(0)
        _check(self.ctx.lib.nrphy_pusch_proc_plan_harq_bytes(self.handle, i, C.byref(soft), C.byref(state)),
               "nrphy_pusch_proc_plan_harq_bytes")
        return int(soft.value), int(state.value)

    def run(self, d_grid, d_harq, d_tb, d_uci_bits, d_result, stream=None):
        """d_harq: the HARQ arena (uint8 / int8); d_tb, d_uci_bits: uint8; d_result: [n] x sizeof(abi.PuschResult) bytes."""
        _check(self.ctx.lib.nrphy_pusch_proc_run(self.handle, _dptr(d_grid), _dptr(d_harq), _dptr(d_tb), _dptr(d_uci_bits),
                                                 _dptr(d_result), _stream(stream)), "nrphy_pusch_proc_run")

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_pusch_proc_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PuschTpPlan(PuschProcPlan):
    """PuschProcPlan made by nrphy_pusch_tp_plan_create: tps is one abi.PuschTpDesc per PDU, or None (a null pointer: the plan of
    nrphy_pusch_evm_plan_create); options is an abi.PuschEvmOptions."""

    def __init__(self, ctx, pdus, tps, options, grid_indices, nof_grids, nof_ports, nof_subc, harq_soft_offsets=None,
                 harq_state_offsets=None, tb_offsets=None, uci_offsets=None):
        self.ctx = ctx
        n = len(pdus)
        arr = (abi.PuschPdu * n)(*pdus)
        tarr = None if tps is None else (abi.PuschTpDesc * n)(*tps)
        gidx = (C.c_uint32 * n)(*grid_indices)
        offs = [None if o is None else (C.c_uint64 * n)(*o) for o in (harq_soft_offsets, harq_state_offsets, tb_offsets, uci_offsets)]
        h = C.c_void_p()
        self.handle = None
        _check(ctx.lib.nrphy_pusch_tp_plan_create(ctx.handle, n, arr, tarr, C.byref(options), gidx, nof_grids, nof_ports, nof_subc, *offs,
                                                  C.byref(h)), "nrphy_pusch_tp_plan_create")
        self.handle = h
        self.n = n


class PuschCsi2Plan:
    """nrphy_pusch_csi2_plan: PuschProcPlan for PDUs of which some carry a CSI part 2 size description (abi.PuschCsi2Desc, one per
    PDU; nof_entries 0 = none).  run() also writes one abi.PuschCsi2Result per PDU; PDU i's part 2 payload goes to byte
    csi2_offsets[i] of d_uci_bits."""

    def __init__(self, ctx, pdus, descs, options, grid_indices, nof_grids, nof_ports, nof_subc, harq_soft_offsets=None,
                 harq_state_offsets=None, tb_offsets=None, uci_offsets=None, csi2_offsets=None):
        self.ctx = ctx
        n = len(pdus)
        arr = (abi.PuschPdu * n)(*pdus)
        darr = (abi.PuschCsi2Desc * n)(*descs)
        gidx = (C.c_uint32 * n)(*grid_indices)
        offs = [None if o is None else (C.c_uint64 * n)(*o)
                for o in (harq_soft_offsets, harq_state_offsets, tb_offsets, uci_offsets, csi2_offsets)]
        h = C.c_void_p()
        _check(ctx.lib.nrphy_pusch_csi2_plan_create(ctx.handle, n, arr, darr, C.byref(options), gidx, nof_grids, nof_ports, nof_subc,
                                                    *offs, C.byref(h)), "nrphy_pusch_csi2_plan_create")
        self.handle = h
        self.n = n

    def run(self, d_grid, d_harq, d_tb, d_uci_bits, d_result, d_csi2_result, stream=None):
        """As PuschProcPlan.run; d_csi2_result: [n] x sizeof(abi.PuschCsi2Result) bytes."""
        _check(self.ctx.lib.nrphy_pusch_csi2_run(self.handle, _dptr(d_grid), _dptr(d_harq), _dptr(d_tb), _dptr(d_uci_bits),
                                                 _dptr(d_result), _dptr(d_csi2_result), _stream(stream)), "nrphy_pusch_csi2_run")

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_pusch_csi2_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pusch_csi2_size(desc, csi_part1_bits):
    """nrphy_pusch_csi2_size: uci_part2_get_size of a CSI part 1 payload (one bit per element), or None for a refused description
    (host only)."""
    bits = np.ascontiguousarray(csi_part1_bits, dtype=np.uint8)
    size = C.c_uint32(0)
    if int(load().nrphy_pusch_csi2_size(C.byref(desc), bits.ctypes.data, bits.size, C.byref(size))) != abi.OK:
        return None
    return int(size.value)


def pusch_csi2_validate(pdu, desc, options, grid_nof_ports, grid_nof_subc):
    """nrphy_pusch_csi2_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_pusch_csi2_validate(C.byref(pdu), C.byref(desc), C.byref(options), grid_nof_ports, grid_nof_subc))


def pusch_csi2_variants(pdu, desc, options, grid_nof_ports, grid_nof_subc):
    """nrphy_pusch_csi2_variants: (sizes, infos) -- the PDU's variant table, sizes[0] = 0, then the distinct non-zero sizes
    ascending, each with its abi.UlschInfo --, or None for a refused PDU (host only)."""
    n = C.c_uint32(0)
    sizes = (C.c_uint32 * abi.PUSCH_CSI2_MAX_VARIANTS)()
    infos = (abi.UlschInfo * abi.PUSCH_CSI2_MAX_VARIANTS)()
    if int(load().nrphy_pusch_csi2_variants(C.byref(pdu), C.byref(desc), C.byref(options), grid_nof_ports, grid_nof_subc, C.byref(n),
                                            sizes, infos)) != abi.OK:
        return None
    return [int(v) for v in sizes[:n.value]], [abi.UlschInfo.from_buffer_copy(infos[k]) for k in range(n.value)]


def pusch_csi2_harq_bytes(pdu, desc, options):
    """nrphy_pusch_csi2_harq_bytes: (soft bytes, state bytes) of the PDU's HARQ blocks (host only)."""
    soft, state = C.c_uint64(0), C.c_uint64(0)
    _check(load().nrphy_pusch_csi2_harq_bytes(C.byref(pdu), C.byref(desc), C.byref(options), C.byref(soft), C.byref(state)),
           "nrphy_pusch_csi2_harq_bytes")
    return int(soft.value), int(state.value)


def ulsch_info(cfg):
    """nrphy_ul_sch_info: the abi.UlschInfo of an abi.UlschInfoCfg, or None for a refused configuration (host only)."""
    out = abi.UlschInfo()
    if int(load().nrphy_ul_sch_info(C.byref(cfg), C.byref(out))) != abi.OK:
        return None
    return out


def pusch_proc_validate(pdu, options, grid_nof_ports, grid_nof_subc):
    """nrphy_pusch_proc_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_pusch_proc_validate(C.byref(pdu), C.byref(options), grid_nof_ports, grid_nof_subc))


def pusch_evm_validate(pdu, options, grid_nof_ports, grid_nof_subc):
    """nrphy_pusch_evm_validate with an abi.PuschEvmOptions: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_pusch_evm_validate(C.byref(pdu), C.byref(options), grid_nof_ports, grid_nof_subc))


def pusch_tp_validate(pdu, tp, options, grid_nof_ports, grid_nof_subc):
    """nrphy_pusch_tp_validate with an abi.PuschTpDesc (or None) and an abi.PuschEvmOptions: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_pusch_tp_validate(C.byref(pdu), None if tp is None else C.byref(tp), C.byref(options), grid_nof_ports,
                                              grid_nof_subc))


def pusch_tp_derive(pdu, tp, options, grid_nof_ports, grid_nof_subc):
    """nrphy_pusch_tp_derive: (abi.PuschProcDerived, abi.PuschChestLowpapr) of a PDU, or None for a refused one (host only)."""
    out, lp = abi.PuschProcDerived(), abi.PuschChestLowpapr()
    if int(load().nrphy_pusch_tp_derive(C.byref(pdu), None if tp is None else C.byref(tp), C.byref(options), grid_nof_ports,
                                        grid_nof_subc, C.byref(out), C.byref(lp))) != abi.OK:
        return None
    return out, lp


def pusch_tp_harq_bytes(pdu, tp, options):
    """nrphy_pusch_tp_harq_bytes: (soft bytes, state bytes) of the PDU's HARQ blocks (host only)."""
    soft, state = C.c_uint64(0), C.c_uint64(0)
    _check(load().nrphy_pusch_tp_harq_bytes(C.byref(pdu), None if tp is None else C.byref(tp), C.byref(options), C.byref(soft),
                                            C.byref(state)), "nrphy_pusch_tp_harq_bytes")
    return int(soft.value), int(state.value)


def pusch_proc_derive(pdu, options, grid_nof_ports, grid_nof_subc):
    """nrphy_pusch_proc_derive: the abi.PuschProcDerived of a PDU, or None for a refused one (host only)."""
    out = abi.PuschProcDerived()
    if int(load().nrphy_pusch_proc_derive(C.byref(pdu), C.byref(options), grid_nof_ports, grid_nof_subc, C.byref(out))) != abi.OK:
        return None
    return out


def pusch_proc_harq_bytes(pdu, options):
    """nrphy_pusch_proc_harq_bytes: (soft bytes, state bytes) of the PDU's HARQ blocks (host only)."""
    soft, state = C.c_uint64(0), C.c_uint64(0)
    _check(load().nrphy_pusch_proc_harq_bytes(C.byref(pdu), C.byref(options), C.byref(soft), C.byref(state)),
           "nrphy_pusch_proc_harq_bytes")
    return int(soft.value), int(state.value)


def ulsch_demux_validate(cfg):
    """nrphy_ulsch_demux_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_ulsch_demux_validate(C.byref(cfg)))


def ulsch_demux_sizes(cfg):
    """nrphy_ulsch_demux_sizes: (nof_sch_bits, nof_codeword_bits), or None for a refused configuration (host only)."""
    s = abi.UlschDemuxSizes()
    if int(load().nrphy_ulsch_demux_sizes(C.byref(cfg), C.byref(s))) != abi.OK:
        return None
    return int(s.nof_sch_bits), int(s.nof_codeword_bits)


def ofh_ul_validate(sections, payload_bytes, nof_grids, grid_nof_ports, grid_nof_subc):
    arr = (abi.OfhUlSection * max(len(sections), 1))(*sections)
    return load().nrphy_ofh_ul_validate(len(sections), arr, payload_bytes, nof_grids, grid_nof_ports, grid_nof_subc)


def ofh_rx_validate(cfg, frames, expects, frames_bytes, nof_grids, grid_nof_ports, grid_nof_subc):
    f_arr = (abi.OfhRxFrame * max(len(frames), 1))(*frames)
    e_arr = (abi.OfhRxExpect * max(len(expects), 1))(*expects)
    return int(load().nrphy_ofh_rx_validate(C.byref(cfg), len(frames), f_arr, len(expects), e_arr, frames_bytes, nof_grids, grid_nof_ports,
                                            grid_nof_subc))


def ofh_dl_fragments(flow):
    """nrphy_ofh_dl_fragments: [(start_prb, nof_prbs, frame_bytes)] of one symbol of the flow, or None for a refused flow."""
    out = (abi.OfhDlFragment * 275)()
    n = C.c_uint32(0)
    if int(load().nrphy_ofh_dl_fragments(C.byref(flow), 275, out, C.byref(n))) != abi.OK:
        return None
    return [(int(f.start_prb), int(f.nof_prbs), int(f.frame_bytes)) for f in out[:n.value]]


def ofh_dl_validate(flows, symbols, nof_grids, grid_nof_ports, grid_nof_subc, frames_bytes, frame_stride):
    f_arr = (abi.OfhDlFlow * max(len(flows), 1))(*flows)
    s_arr = (abi.OfhDlSymbol * max(len(symbols), 1))(*symbols)
    return int(load().nrphy_ofh_dl_validate(len(flows), f_arr, len(symbols), s_arr, nof_grids, grid_nof_ports, grid_nof_subc,
                                            frames_bytes, frame_stride))


def ofh_ul_prach_validate(sections, payload_bytes, symbols_elems):
    arr = (abi.OfhUlPrachSection * max(len(sections), 1))(*sections)
    return load().nrphy_ofh_ul_prach_validate(len(sections), arr, payload_bytes, symbols_elems)


def uci_decoder_validate(cfg):
    """nrphy_uci_decoder_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_uci_decoder_validate(C.byref(cfg)))


class PrachDemodPlan:
    """nrphy_prach_demod_plan: item i reads port p's complex64 samples at element in_offsets[i] + p * in_port_stride and writes
    element out_offsets[i] + p * port_stride + fd * fd_stride + td * td_stride + s * symbol_stride + k of the symbols."""

    def __init__(self, ctx, cfgs, in_offsets, in_port_stride, out_offsets, port_stride, fd_stride, td_stride, symbol_stride):
        self.ctx = ctx
        self.handle = None
        n = len(cfgs)
        arr = (abi.PrachDemodCfg * n)(*cfgs)
        ins = (C.c_uint64 * n)(*in_offsets)
        outs = (C.c_uint64 * n)(*out_offsets)
        h = C.c_void_p()
        _check(ctx.lib.nrphy_prach_demod_plan_create(ctx.handle, n, arr, ins, in_port_stride, outs, port_stride, fd_stride, td_stride,
                                                     symbol_stride, C.byref(h)), "nrphy_prach_demod_plan_create")
        self.handle = h
        self.n = n

    def run(self, d_samples, d_symbols, stream=None):
        _check(self.ctx.lib.nrphy_prach_demod_run(self.handle, _dptr(d_samples), _dptr(d_symbols), _stream(stream)),
               "nrphy_prach_demod_run")

    def run_iq(self, d_iq, d_symbols, iq_format=abi.IQ_CF32, iq_scale=1.0, stream=None):
        """nrphy_prach_window_demod_run: the same from complex64 or (abi.IQ_CI16) int16-pair samples; returns the status."""
        return int(self.ctx.lib.nrphy_prach_window_demod_run(self.handle, _dptr(d_iq), iq_format, iq_scale, _dptr(d_symbols),
                                                             _stream(stream)))

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_prach_demod_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prach_demod_validate(cfg):
    """nrphy_prach_demod_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_prach_demod_validate(C.byref(cfg)))


def prach_demod_sizes(cfg):
    """nrphy_prach_demod_sizes: abi.PrachDemodSizes, or None for a refused configuration (host only)."""
    sz = abi.PrachDemodSizes()
    return sz if int(load().nrphy_prach_demod_sizes(C.byref(cfg), C.byref(sz))) == abi.OK else None


def prach_validate(cfg):
    """nrphy_prach_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_prach_validate(C.byref(cfg)))


def prach_threshold(cfg):
    """nrphy_prach_threshold: (threshold, win_margin, flag) of the table's exact row, or None where it has none (host only)."""
    th, margin, flag = C.c_float(), C.c_uint32(), C.c_uint32()
    if int(load().nrphy_prach_threshold(C.byref(cfg), C.byref(th), C.byref(margin), C.byref(flag))) != abi.OK:
        return None
    return float(th.value), int(margin.value), int(flag.value)


def prach_window_width(cfg):
    """nrphy_prach_window_width: correlation samples per metric window, 0 for a refused configuration (host only)."""
    return int(load().nrphy_prach_window_width(C.byref(cfg)))


def pucch_validate(cfg, grid_nof_ports, grid_nof_subc):
    """nrphy_pucch_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_pucch_validate(C.byref(cfg), grid_nof_ports, grid_nof_subc))


def pf2_validate(cfg, grid_nof_ports, grid_nof_subc):
    """nrphy_pf2_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_pf2_validate(C.byref(cfg), grid_nof_ports, grid_nof_subc))


def srs_validate(cfg, grid_nof_ports, grid_nof_subc):
    """nrphy_srs_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_srs_validate(C.byref(cfg), grid_nof_ports, grid_nof_subc))


def srs_info(cfg, antenna_port):
    """nrphy_srs_info: get_srs_information's values as a dict, or None for a configuration out of range (host only)."""
    v = [C.c_uint32() for _ in range(5)]
    if load().nrphy_srs_info(C.byref(cfg), antenna_port, *[C.byref(x) for x in v]) != abi.OK:
        return None
    return dict(zip(("sequence_length", "initial_subcarrier", "n_cs", "n_cs_max", "u"), (int(x.value) for x in v)))


def pf2_sizes(cfg):
    """nrphy_pf2_sizes: (E soft bits, A payload bits), or None for a configuration the validator refuses (host only)."""
    e, a = C.c_uint32(), C.c_uint32()
    if load().nrphy_pf2_sizes(C.byref(cfg), C.byref(e), C.byref(a)) != abi.OK:
        return None
    return int(e.value), int(a.value)


def pusch_chest_validate_ex(cfg, lowpapr, grid_nof_ports, grid_nof_subc):
    """nrphy_pusch_chest_validate_ex with an abi.PuschChestLowpapr (or None): abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_pusch_chest_validate_ex(C.byref(cfg), None if lowpapr is None else C.byref(lowpapr), grid_nof_ports,
                                                    grid_nof_subc))


def pusch_chest_validate(cfg, grid_nof_ports, grid_nof_subc):
    """nrphy_pusch_chest_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_pusch_chest_validate(C.byref(cfg), grid_nof_ports, grid_nof_subc))


def pusch_demod_validate(cfg, grid_nof_ports, grid_nof_subc):
    """nrphy_pusch_demod_validate: abi.OK or abi.ERR_ARGUMENT (host only)."""
    return int(load().nrphy_pusch_demod_validate(C.byref(cfg), grid_nof_ports, grid_nof_subc))


def pusch_demod_validate_ex(cfg, grid_nof_ports, grid_nof_subc, features):
    """nrphy_pusch_demod_validate_ex: the validator with a feature mask (abi.PUSCH_DEMOD_*); host only."""
    return int(load().nrphy_pusch_demod_validate_ex(C.byref(cfg), grid_nof_ports, grid_nof_subc, features))


def transform_precoding_nof_prb_valid(nof_prb):
    """nrphy_transform_precoding_nof_prb_valid: whether 12 * nof_prb is a transform-precoding size (host only)."""
    return bool(load().nrphy_transform_precoding_nof_prb_valid(nof_prb))


def pusch_demod_codeword_bits(cfg):
    """G = data RE x layers x qm (host only)."""
    return int(load().nrphy_pusch_demod_codeword_bits(C.byref(cfg)))


class PdschAsyncQueue:
    """nrphy_pdsch_async: up to `depth` PDUs in flight through the host-span seam, completion on a runtime thread."""

    def __init__(self, ctx, depth, nof_ports, nof_subc, max_tb_bytes):
        self.ctx, self.nof_ports, self.nof_subc = ctx, nof_ports, nof_subc
        h = C.c_void_p()
        _check(ctx.lib.nrphy_pdsch_async_create(ctx.handle, depth, nof_ports, nof_subc, max_tb_bytes, C.byref(h)),
               "nrphy_pdsch_async_create")
        self.handle = h
        self._keep = []

    def submit(self, pdu, tb, on_done):
        """on_done(status, grid) runs on a HIP runtime thread; grid is a copy [nof_ports][14][nof_subc][2] uint16.
        Returns False when `depth` PDUs are in flight (retry after a completion)."""
        shape = (self.nof_ports, 14, self.nof_subc, 2)

        def trampoline(user, status, grid_ptr):
            grid = np.ctypeslib.as_array(C.cast(grid_ptr, C.POINTER(C.c_uint16)), shape=shape).copy() if status == 0 else None
            on_done(status, grid)

        cb = abi.PDSCH_DONE_FN(trampoline)
        self._keep.append(cb)
        tb = np.ascontiguousarray(tb, dtype=np.uint8)
        rc = self.ctx.lib.nrphy_pdsch_async_submit(self.handle, C.byref(pdu), tb.ctypes.data, cb, None)
        if rc == abi.ERR_CAPACITY:
            self._keep.pop()
            return False
        _check(rc, "nrphy_pdsch_async_submit")
        return True

    def submit_slot(self, pdus, tbs, on_done):
        """All PDUs of one slot as one operation (nrphy_pdsch_async_submit_slot); otherwise as submit()."""
        shape = (self.nof_ports, 14, self.nof_subc, 2)

        def trampoline(user, status, grid_ptr):
            grid = np.ctypeslib.as_array(C.cast(grid_ptr, C.POINTER(C.c_uint16)), shape=shape).copy() if status == 0 else None
            on_done(status, grid)

        cb = abi.PDSCH_DONE_FN(trampoline)
        self._keep.append(cb)
        n = len(pdus)
        arr = (abi.PdschPdu * n)(*pdus)
        keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in tbs]
        ptrs = (C.c_void_p * n)(*[t.ctypes.data for t in keep])
        rc = self.ctx.lib.nrphy_pdsch_async_submit_slot(self.handle, n, arr, ptrs, cb, None)
        if rc == abi.ERR_CAPACITY:
            self._keep.pop()
            return False
        _check(rc, "nrphy_pdsch_async_submit_slot")
        return True

    def wait(self):
        _check(self.ctx.lib.nrphy_pdsch_async_wait(self.handle), "nrphy_pdsch_async_wait")
        self._keep.clear()

    def wait_slot(self):
        """Blocks while all `depth` operations are in flight."""
        _check(self.ctx.lib.nrphy_pdsch_async_wait_slot(self.handle), "nrphy_pdsch_async_wait_slot")

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_pdsch_async_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SlotPool:
    """What DlSlotPool and UlSlots share: the per-slot calls that differ in the C prefix alone (`_PREFIX`: nrphy_dl_slot /
    nrphy_ul_slot), the two calls on the pool itself (`_WAIT_FREE`, `_DESTROY`: their C names) and the done-callback trampolines
    (`_DONE_FN`), kept alive until their slot is closed."""
    _PREFIX = _WAIT_FREE = _DESTROY = _DONE_FN = None

    def _adopt(self, handle):
        self.handle = handle
        self._keep = {}

    def _call(self, name, *args):
        return getattr(self.ctx.lib, self._PREFIX + name)(self.handle, *args)

    def _done_callback(self, sid, on_done):
        """The C callback that runs on_done(status, slot_id), or None."""
        if on_done is None:
            return None
        cb = self._DONE_FN(lambda user, status, slot_id: on_done(status, slot_id))
        self._keep[sid] = cb
        return cb

    def close(self, sid):
        _check(self._call("_close", sid), self._PREFIX + "_close")
        self._keep.pop(sid, None)

    def wait_free(self):
        _check(getattr(self.ctx.lib, self._WAIT_FREE)(self.handle), self._WAIT_FREE)

    def poll(self, sid):
        return int(self._call("_poll", sid))

    def wait(self, sid):
        return int(self._call("_wait", sid))

    def read_grid(self, sid):
        grid = np.zeros((self.nof_ports, 14, self.nof_subc, 2), dtype=np.uint16)
        _check(self._call("_read_grid", sid, grid.ctypes.data), self._PREFIX + "_read_grid")
        return grid

    def destroy(self):
        if self.handle:
            getattr(self.ctx.lib, self._DESTROY)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class DlSlotPool(_SlotPool):
    """nrphy_dl_slots: the downlink slot pipeline -- every channel of a slot written into ONE device-resident grid, the
    whole slot modulated at grid hand-over, IQ served from pinned host memory (pdxch_processor_impl.cpp:47-112)."""
    _PREFIX, _DONE_FN = "nrphy_dl_slot", abi.DL_SLOT_DONE_FN
    _WAIT_FREE, _DESTROY = "nrphy_dl_slots_wait_free", "nrphy_dl_slots_destroy"

    def __init__(self, ctx, ofdm_cfg, nof_ports, depth, max_tb_bytes, wire_cfg=None):
        self.ctx, self.cfg, self.nof_ports = ctx, ofdm_cfg, nof_ports
        self.nof_subc = 12 * ofdm_cfg.bw_rb
        c = abi.DlSlotsCfg()
        c.ofdm, c.nof_ports, c.depth, c.max_tb_bytes = ofdm_cfg, nof_ports, depth, max_tb_bytes
        c.iq_format = 0 if wire_cfg is None else 1
        if wire_cfg is not None:
            c.wire = wire_cfg
        self.wire = wire_cfg is not None
        h = C.c_void_p()
        _check(ctx.lib.nrphy_dl_slots_create(ctx.handle, C.byref(c), C.byref(h)), "nrphy_dl_slots_create")
        self._adopt(h)

    def open(self):
        """A free slot with an all-zero grid, or None when all `depth` slots are open."""
        sid = C.c_uint32()
        rc = self.ctx.lib.nrphy_dl_slot_open(self.handle, C.byref(sid))
        if rc == abi.ERR_CAPACITY:
            return None
        _check(rc, "nrphy_dl_slot_open")
        return sid.value

    def pdsch(self, sid, pdus, tbs):
        n = len(pdus)
        arr = (abi.PdschPdu * n)(*pdus)
        keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in tbs]
        ptrs = (C.c_void_p * n)(*[t.ctypes.data for t in keep])
        return self.ctx.lib.nrphy_dl_slot_pdsch(self.handle, sid, n, arr, ptrs)

    def pdcch(self, sid, pdus):
        arr = (abi.PdcchPdu * len(pdus))(*pdus)
        _check(self.ctx.lib.nrphy_dl_slot_pdcch(self.handle, sid, len(pdus), arr), "nrphy_dl_slot_pdcch")

    def ssb(self, sid, pdus):
        arr = (abi.SsbPdu * len(pdus))(*pdus)
        _check(self.ctx.lib.nrphy_dl_slot_ssb(self.handle, sid, len(pdus), arr), "nrphy_dl_slot_ssb")

    def csi_rs(self, sid, cfgs):
        arr = (abi.CsiRsCfg * len(cfgs))(*cfgs)
        _check(self.ctx.lib.nrphy_dl_slot_csi_rs(self.handle, sid, len(cfgs), arr), "nrphy_dl_slot_csi_rs")

    def put(self, sid, entries):
        arr = (abi.GridRe * len(entries))(*entries)
        _check(self.ctx.lib.nrphy_dl_slot_put(self.handle, sid, len(entries), arr), "nrphy_dl_slot_put")

    def load_grid(self, sid, grid):
        grid = np.ascontiguousarray(grid, dtype=np.uint16)
        assert grid.size == self.nof_ports * 14 * self.nof_subc * 2
        _check(self.ctx.lib.nrphy_dl_slot_load_grid(self.handle, sid, grid.ctypes.data), "nrphy_dl_slot_load_grid")

    def modulate(self, sid, subframe_slot_index, on_done=None):
        """on_done(status, slot_id) runs on a HIP runtime thread when the slot's IQ is in pinned host memory."""
        return self.ctx.lib.nrphy_dl_slot_modulate(self.handle, sid, subframe_slot_index, self._done_callback(sid, on_done), None)

    def iq(self, sid, port):
        """A copy of the slot's samples of `port`: complex64, or int16 pairs [n][2] for a wire-format pool."""
        n = C.c_uint32()
        ptr = self.ctx.lib.nrphy_dl_slot_iq(self.handle, sid, port, C.byref(n))
        assert ptr
        if self.wire:
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int16)), shape=(n.value, 2)).copy()
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(n.value, 2)).copy().view(np.complex64).reshape(-1)

    def amplitude_stats(self, sid, port):
        """Wire-format pools: a copy of the amplitude controller's raw measurements of the slot's buffer of `port`."""
        p = self.ctx.lib.nrphy_dl_slot_amplitude_stats(self.handle, sid, port)
        assert p
        st = abi.AmplitudeStats()
        C.memmove(C.byref(st), p, C.sizeof(abi.AmplitudeStats))
        return st


class UlSlots(_SlotPool):
    """nrphy_ul_slots: the uplink slot pipeline -- samples demodulated run by run into ONE device-resident grid, every receiver
    of the slot on that grid, the results served from pinned host memory (puxch_processor_impl.cpp:30-97,
    uplink_processor_impl.cpp:86-170).  The calls that the order rules may refuse return the status; the others raise."""
    _PREFIX, _DONE_FN = "nrphy_ul_slot", abi.UL_SLOT_DONE_FN
    _WAIT_FREE, _DESTROY = "nrphy_ul_slots_wait_free", "nrphy_ul_slots_destroy"

    def __init__(self, ctx, ofdm_cfg, nof_ports, depth, iq_format=abi.IQ_CF32, iq_scale=1.0, window_offset=0, max_pusch=0,
                 max_pucch=0, max_pf2=0, max_srs=0, max_tb_bytes=0, max_uci_bits=0, d_harq=None):
        self.ctx, self.cfg, self.nof_ports = ctx, ofdm_cfg, nof_ports
        self.nof_subc = 12 * ofdm_cfg.bw_rb
        self.iq_format = iq_format
        c = abi.UlSlotsCfg()
        c.ofdm, c.nof_ports, c.depth, c.iq_format, c.iq_scale, c.window_offset = ofdm_cfg, nof_ports, depth, iq_format, iq_scale, window_offset
        c.max_pusch, c.max_pucch, c.max_pf2, c.max_srs = max_pusch, max_pucch, max_pf2, max_srs
        c.max_tb_bytes, c.max_uci_bits = max_tb_bytes, max_uci_bits
        self._harq = d_harq  # the caller's arena stays alive with the pool
        h = C.c_void_p()
        _check(ctx.lib.nrphy_ul_slots_create(ctx.handle, C.byref(c), _dptr(d_harq), C.byref(h)), "nrphy_ul_slots_create")
        self._adopt(h)

    def open(self, subframe_slot_index=0):
        """A free slot with an all-zero grid, or None when all `depth` slots are open."""
        sid = C.c_uint32()
        rc = self.ctx.lib.nrphy_ul_slot_open(self.handle, subframe_slot_index, C.byref(sid))
        if rc == abi.ERR_CAPACITY:
            return None
        _check(rc, "nrphy_ul_slot_open")
        return sid.value

    def samples(self, sid, first_symbol, nof_symbols, port_samples):
        """port_samples: per port the samples of the run, complex64 [n] or (abi.IQ_CI16 pools) int16 [n][2]."""
        dtype = np.int16 if self.iq_format == abi.IQ_CI16 else np.complex64
        keep = [np.ascontiguousarray(x, dtype=dtype) for x in port_samples]
        assert len(keep) == self.nof_ports
        ptrs = (C.c_void_p * len(keep))(*[x.ctypes.data for x in keep])
        return int(self.ctx.lib.nrphy_ul_slot_samples(self.handle, sid, first_symbol, nof_symbols, ptrs))

    def load_grid(self, sid, grid):
        grid = np.ascontiguousarray(grid, dtype=np.uint16)
        assert grid.size == self.nof_ports * 14 * self.nof_subc * 2
        return int(self.ctx.lib.nrphy_ul_slot_load_grid(self.handle, sid, grid.ctypes.data))

    def device_grid(self, sid):
        return self.ctx.lib.nrphy_ul_slot_device_grid(self.handle, sid)

    def stream(self, sid):
        return self.ctx.lib.nrphy_ul_slot_stream(self.handle, sid)

    def symbols_written(self, sid, upto):
        return int(self.ctx.lib.nrphy_ul_slot_symbols_written(self.handle, sid, upto))

    def pusch(self, sid, pdus, options, harq_soft_offsets=None, harq_state_offsets=None):
        n = len(pdus)
        arr = (abi.PuschPdu * n)(*pdus)
        soft = (C.c_uint64 * n)(*harq_soft_offsets) if harq_soft_offsets is not None else None
        state = (C.c_uint64 * n)(*harq_state_offsets) if harq_state_offsets is not None else None
        return int(self.ctx.lib.nrphy_ul_slot_pusch(self.handle, sid, n, arr, C.byref(options), soft, state))

    def pusch_evm(self, sid, pdus, options, harq_soft_offsets=None, harq_state_offsets=None):
        """pusch() with an abi.PuschEvmOptions (nrphy_pusch_evm_slot); the results append to the same list."""
        n = len(pdus)
        arr = (abi.PuschPdu * n)(*pdus)
        soft = (C.c_uint64 * n)(*harq_soft_offsets) if harq_soft_offsets is not None else None
        state = (C.c_uint64 * n)(*harq_state_offsets) if harq_state_offsets is not None else None
        return int(self.ctx.lib.nrphy_pusch_evm_slot(self.handle, sid, n, arr, C.byref(options), soft, state))

    def pusch_tp(self, sid, pdus, tps, options, harq_soft_offsets=None, harq_state_offsets=None):
        """pusch_evm() with one abi.PuschTpDesc per PDU, or None (nrphy_pusch_tp_slot); the results append to the same list."""
        n = len(pdus)
        arr = (abi.PuschPdu * n)(*pdus)
        tarr = None if tps is None else (abi.PuschTpDesc * n)(*tps)
        soft = (C.c_uint64 * n)(*harq_soft_offsets) if harq_soft_offsets is not None else None
        state = (C.c_uint64 * n)(*harq_state_offsets) if harq_state_offsets is not None else None
        return int(self.ctx.lib.nrphy_pusch_tp_slot(self.handle, sid, n, arr, tarr, C.byref(options), soft, state))

    def pucch(self, sid, cfgs):
        arr = (abi.PucchCfg * len(cfgs))(*cfgs)
        return int(self.ctx.lib.nrphy_ul_slot_pf01(self.handle, sid, len(cfgs), arr))

    def pf2(self, sid, cfgs):
        arr = (abi.Pf2Cfg * len(cfgs))(*cfgs)
        return int(self.ctx.lib.nrphy_ul_slot_pf2(self.handle, sid, len(cfgs), arr))

    def srs(self, sid, cfgs):
        arr = (abi.SrsCfg * len(cfgs))(*cfgs)
        return int(self.ctx.lib.nrphy_ul_slot_srs(self.handle, sid, len(cfgs), arr))

    def finish(self, sid, on_done=None):
        """on_done(status, slot_id) runs on a HIP runtime thread when the slot's results are in pinned host memory."""
        return int(self.ctx.lib.nrphy_ul_slot_finish(self.handle, sid, self._done_callback(sid, on_done), None))

    def _records(self, fn, sid, cls):
        n = C.c_uint32()
        ptr = fn(self.handle, sid, C.byref(n))
        assert ptr
        out = (cls * n.value)()
        C.memmove(out, ptr, C.sizeof(cls) * n.value)
        return list(out)

    def _bytes(self, fn, sid, i):
        n = C.c_uint32()
        ptr = fn(self.handle, sid, i, C.byref(n))
        assert ptr
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint8)

    def pusch_results(self, sid):
        """Copies of the slot's abi.PuschResult records, in call order."""
        return self._records(self.ctx.lib.nrphy_ul_slot_pusch_results, sid, abi.PuschResult)

    def tb(self, sid, i):
        return self._bytes(self.ctx.lib.nrphy_ul_slot_tb, sid, i)

    def uci_bits(self, sid, i):
        return self._bytes(self.ctx.lib.nrphy_ul_slot_pusch_uci, sid, i)

    def pucch_results(self, sid):
        return self._records(self.ctx.lib.nrphy_ul_slot_pf01_results, sid, abi.PucchResult)

    def pf2_result(self, sid, i):
        """(message bits, status, abi.Pf2Csi) of the slot's i-th format 2 PUCCH."""
        msg, n, status, csi = C.c_void_p(), C.c_uint32(), C.c_uint32(), abi.Pf2Csi()
        _check(self.ctx.lib.nrphy_ul_slot_format2_results(self.handle, sid, i, C.byref(msg), C.byref(n), C.byref(status), C.byref(csi)),
               "nrphy_ul_slot_format2_results")
        bits = np.ctypeslib.as_array(C.cast(msg, C.POINTER(C.c_uint8)), shape=(n.value,)).copy()
        return bits, int(status.value), csi

    def srs_results(self, sid):
        return self._records(self.ctx.lib.nrphy_ul_slot_sounding_results, sid, abi.SrsResult)


class PrachWindows(_SlotPool):
    """nrphy_prach_windows: the PRACH window pipeline -- the samples of a window collected run by run in the radio's format, the
    demodulator and the detector on the window's device-resident prach_buffer, the detections served from pinned host memory
    (prach_processor_worker.cpp:31-162).  The calls that the order rules may refuse return the status; the others raise."""
    _PREFIX, _DONE_FN = "nrphy_prach_window", abi.PRACH_WINDOW_DONE_FN
    _WAIT_FREE, _DESTROY = "nrphy_prach_windows_wait_free", "nrphy_prach_windows_destroy"

    def __init__(self, ctx, srate_hz, nof_radio_ports, depth, max_window_samples, iq_format=abi.IQ_CF32, iq_scale=1.0, max_ports=1,
                 max_td_occasions=1, max_fd_occasions=1):
        self.ctx, self.nof_radio_ports, self.iq_format = ctx, nof_radio_ports, iq_format
        c = abi.PrachWindowsCfg()
        c.srate_hz, c.nof_radio_ports, c.depth, c.iq_format, c.max_window_samples = srate_hz, nof_radio_ports, depth, iq_format, max_window_samples
        c.iq_scale, c.max_ports, c.max_td_occasions, c.max_fd_occasions = iq_scale, max_ports, max_td_occasions, max_fd_occasions
        h = C.c_void_p()
        _check(ctx.lib.nrphy_prach_windows_create(ctx.handle, C.byref(c), C.byref(h)), "nrphy_prach_windows_create")
        self._adopt(h)
        self._shape = {}

    def open(self, demod_cfg, radio_ports, detect_cfg, on_done=None):
        """(status, window id or None).  on_done(status, window_id) runs on a HIP runtime thread when the window's detections are
        in pinned host memory.  radio_ports: per PRACH port the radio port its samples come from."""
        wid = C.c_uint32()
        cb = self._done_callback(None, on_done)  # registered under the id once the call has given it
        ports = (C.c_uint32 * max(len(radio_ports), 1))(*radio_ports)
        rc = int(self.ctx.lib.nrphy_prach_window_open(self.handle, C.byref(demod_cfg), ports, C.byref(detect_cfg), cb, None, C.byref(wid)))
        self._keep.pop(None, None)
        if rc != abi.OK:
            return rc, None
        self._keep[wid.value] = cb
        sz = prach_demod_sizes(demod_cfg)
        self._shape[wid.value] = (demod_cfg.nof_rx_ports, demod_cfg.nof_td_occasions, demod_cfg.nof_fd_occasions, sz.nof_symbols,
                                  sz.sequence_length)
        return rc, wid.value

    def samples(self, wid, radio_port_samples):
        """radio_port_samples: per RADIO port the samples of the run, complex64 [n] or (abi.IQ_CI16 pools) int16 [n][2]; None for
        a port no PRACH port maps to.  Returns (status, taken)."""
        dtype = np.int16 if self.iq_format == abi.IQ_CI16 else np.complex64
        keep = [None if x is None else np.ascontiguousarray(x, dtype=dtype) for x in radio_port_samples]
        assert len(keep) == self.nof_radio_ports
        n = {x.size // (2 if self.iq_format == abi.IQ_CI16 else 1) for x in keep if x is not None}
        assert len(n) == 1
        ptrs = (C.c_void_p * len(keep))(*[None if x is None else x.ctypes.data for x in keep])
        taken = C.c_uint32()
        rc = int(self.ctx.lib.nrphy_prach_window_samples(self.handle, wid, n.pop(), ptrs, C.byref(taken)))
        return rc, int(taken.value)

    def read_grid(self, sid):
        raise AttributeError("a PRACH window has no grid: read_buffer")

    def device_buffer(self, wid):
        return self.ctx.lib.nrphy_prach_window_device_buffer(self.handle, wid)

    def stream(self, wid):
        return self.ctx.lib.nrphy_prach_window_stream(self.handle, wid)

    def buffer_written(self, wid):
        return int(self.ctx.lib.nrphy_prach_window_buffer_written(self.handle, wid))

    def read_buffer(self, wid):
        """Blocking: the window's prach_buffer [ports][td][fd][symbols][L_RA] complex64."""
        out = np.zeros(self._shape[wid], np.complex64)
        _check(self.ctx.lib.nrphy_prach_window_read_buffer(self.handle, wid, out.ctypes.data), "nrphy_prach_window_read_buffer")
        return out

    def results(self, wid):
        """Copies of the window's abi.PrachResult headers, one per (td, fd) occasion, td outer."""
        n = C.c_uint32()
        ptr = self.ctx.lib.nrphy_prach_window_results(self.handle, wid, C.byref(n))
        assert ptr
        out = (abi.PrachResult * n.value)()
        C.memmove(out, ptr, C.sizeof(abi.PrachResult) * n.value)
        return list(out)

    def preambles(self, wid, occasion):
        """A copy of the 64 abi.PrachPreamble records of one occasion."""
        ptr = self.ctx.lib.nrphy_prach_window_preambles(self.handle, wid, occasion)
        assert ptr
        out = (abi.PrachPreamble * abi.PRACH_MAX_PREAMBLES)()
        C.memmove(out, ptr, C.sizeof(out))
        return out

    def plans_made(self):
        return int(self.ctx.lib.nrphy_prach_windows_plans_made(self.handle))


class OfdmPlan:
    """nrphy_ofdm_plan: ofdm_modulator_configuration + port count."""

    def __init__(self, ctx, cfg, nof_ports):
        self.ctx = ctx
        self.cfg = cfg
        self.nof_ports = nof_ports
        h = C.c_void_p()
        _check(ctx.lib.nrphy_ofdm_plan_create(ctx.handle, C.byref(cfg), nof_ports, C.byref(h)),
               "nrphy_ofdm_plan_create")
        self.handle = h
        self.slot_stride = int(ctx.lib.nrphy_ofdm_plan_slot_stride(h))

    def run(self, nof_grids, d_grid, d_iq, d_slot_index=None, stream=None):
        _check(self.ctx.lib.nrphy_ofdm_run(self.handle, nof_grids, _dptr(d_grid), _dptr(d_slot_index), _dptr(d_iq),
                                           _stream(stream)), "nrphy_ofdm_run")

    def run_ci16(self, nof_grids, d_grid, wire_cfg, d_iq16, d_slot_index=None, d_stats=None, stream=None):
        """nrphy_ofdm_run with the amplitude controller and the complex int16 conversion fused into the store."""
        _check(self.ctx.lib.nrphy_ofdm_run_ci16(self.handle, nof_grids, _dptr(d_grid), _dptr(d_slot_index), C.byref(wire_cfg),
                                                _dptr(d_iq16), _dptr(d_stats), _stream(stream)), "nrphy_ofdm_run_ci16")

    def enable_timing(self, max_runs, stride=1):
        _check(self.ctx.lib.nrphy_ofdm_plan_enable_timing(self.handle, max_runs), "nrphy_ofdm_plan_enable_timing")
        _check(self.ctx.lib.nrphy_ofdm_plan_timing_stride(self.handle, stride), "nrphy_ofdm_plan_timing_stride")

    def kernel_time(self):
        ms = C.c_float(0)
        n = C.c_uint32(0)
        _check(self.ctx.lib.nrphy_ofdm_plan_kernel_time(self.handle, C.byref(ms), C.byref(n)),
               "nrphy_ofdm_plan_kernel_time")
        return float(ms.value), int(n.value)

    def modulate_symbol_host(self, grid, port, symbol_index):
        grid = np.ascontiguousarray(grid, dtype=np.uint16)
        n = symbol_size(self.cfg, symbol_index)
        out = np.zeros(n, np.complex64)
        _check(self.ctx.lib.nrphy_ofdm_modulate_symbol_host(self.handle, grid.ctypes.data, port, symbol_index,
                                                            out.ctypes.data, n), "nrphy_ofdm_modulate_symbol_host")
        return out

    def demod_run(self, nof_grids, d_iq, d_grid, d_slot_index=None, window_offset=0, stream=None):
        """ofdm_slot_demodulator::demodulate for every port of nof_grids slots (device buffers)."""
        _check(self.ctx.lib.nrphy_ofdm_demod_run(self.handle, nof_grids, _dptr(d_iq), _dptr(d_slot_index),
                                                 window_offset, _dptr(d_grid), _stream(stream)), "nrphy_ofdm_demod_run")

    def demod_symbols(self, nof_grids, d_iq, d_grid, first_symbol, nof_symbols, iq_format=abi.IQ_CF32, iq_scale=1.0,
                      d_slot_index=None, window_offset=0, stream=None):
        """puxch_processor_impl::process_symbol for a run of symbols: demod_run over symbols [first_symbol, first_symbol +
        nof_symbols) only, from complex float or (abi.IQ_CI16) complex int16 samples widened by 1 / iq_scale.  Returns the
        status."""
        return int(self.ctx.lib.nrphy_ofdm_demod_symbols(self.handle, nof_grids, _dptr(d_iq), iq_format, iq_scale, _dptr(d_slot_index),
                                                         first_symbol, nof_symbols, window_offset, _dptr(d_grid), _stream(stream)))

    def demodulate_slot_host(self, iq, slot_index, window_offset=0):
        """Host-span form: iq [nof_ports][slot samples] complex64 -> grid [nof_ports][14][12*bw_rb][2] uint16."""
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        grid = np.zeros((self.nof_ports, 14, 12 * self.cfg.bw_rb, 2), np.uint16)
        _check(self.ctx.lib.nrphy_ofdm_demodulate_slot_host(self.handle, iq.ctypes.data, slot_index, window_offset,
                                                            grid.ctypes.data), "nrphy_ofdm_demodulate_slot_host")
        return grid

    def demodulate_symbol_host(self, samples, symbol_index, window_offset=0):
        """ofdm_symbol_demodulator::demodulate for one symbol of one port -> [12*bw_rb][2] uint16."""
        samples = np.ascontiguousarray(samples, dtype=np.complex64)
        row = np.zeros((12 * self.cfg.bw_rb, 2), np.uint16)
        _check(self.ctx.lib.nrphy_ofdm_demodulate_symbol_host(self.handle, samples.ctypes.data, samples.size,
                                                              symbol_index, window_offset, row.ctypes.data),
               "nrphy_ofdm_demodulate_symbol_host")
        return row

    def modulate_slot_host(self, grid, slot_index, out=None):
        """ofdm_slot_modulator::modulate for every port of one host grid: [nof_ports][slot samples] complex64."""
        grid = np.ascontiguousarray(grid, dtype=np.uint16)
        n = slot_size(self.cfg, slot_index)
        if out is None:
            out = np.zeros((self.nof_ports, n), np.complex64)
        _check(self.ctx.lib.nrphy_ofdm_modulate_slot_host(self.handle, grid.ctypes.data, slot_index, out.ctypes.data),
               "nrphy_ofdm_modulate_slot_host")
        return out

    def close(self):
        if self.handle:
            self.ctx.lib.nrphy_ofdm_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- host-only helpers (no GPU needed) ---------------------------------------------------------------------------
def validate(pdu):
    return int(load().nrphy_pdsch_validate(C.byref(pdu)))


def derive(pdu):
    d = abi.PdschDerived()
    _check(load().nrphy_pdsch_derive(C.byref(pdu), C.byref(d)), "nrphy_pdsch_derive")
    return d.as_dict()


def tbs_calculate(nof_symb_sh, nof_dmrs_prb, nof_oh_prb, qm, rate_x1024, nof_layers, n_prb):
    return int(load().nrphy_tbs_calculate(nof_symb_sh, nof_dmrs_prb, nof_oh_prb, qm, float(rate_x1024), nof_layers,
                                          n_prb))


def symbol_size(cfg, symbol_index):
    return int(load().nrphy_ofdm_symbol_size(C.byref(cfg), symbol_index))


def slot_size(cfg, slot_index):
    return int(load().nrphy_ofdm_slot_size(C.byref(cfg), slot_index))
