"""BatchDecoder -- host mirror of the reference's frame-level entry points for a batch of
streams.  One object owns the per-stream state ({cur, prev, prev_enhanced} + the per-stream
RNG state that the reference keeps thread-local) in HBM and feeds frames through the C-ABI
launcher.  torch is used for device memory and streams only.

Reference interface mirrored (include/mbelib-neo/mbelib.h):
  mbe_initMbeParms                      -> BatchDecoder(...)            (state defaults)
  mbe_setThreadRngSeed                  -> seeds=...                    (per stream)
  mbe_processImbe7200x4400Frame[f]      -> decode(frames, T)            codec=IMBE
  mbe_processAmbe3600x2450Frame[f]      -> decode(frames, T)            codec=AMBE
  mbe_decode*Frame                      -> fec(frames)
  mbe_decode*Frame, the caller's keystream XOR, mbe_process*Dataf -> decode / decode_soft / decode_ragged(..., keystream=rows)
Beyond the reference: compand(pcm16, law) -- the int16 rows of a decode as G.711 bytes (include/mbx_pcm8.h);
mixdown(pcm16, plan, form) -- the rows summed into talkgroup buses, a gain per input (include/mbx_mixdown.h);
levels(pcm16) -- a level record per row, and mixdown_gated(pcm16, plan, form, open_peak, loudest_n) -- the buses of the open / the N
loudest inputs (include/mbx_levels.h); mixdown_held(pcm16, plan, state, hold, form) -- the same with hysteresis, hang time and ramps,
a state record per input kept on the device (include/mbx_hold.h); agc(pcm16, T, state, agc) -- the rows levelled by a per-stream
automatic gain, a state record per stream kept on the device (include/mbx_agc.h); mixdown_sums / mixdown_gated_sums /
mixdown_held_sums -- the buses as int32 sums in front of the clamp, and bus_limit(sums, T, state, limit, form) -- those sums under a
look-ahead peak limiter, a state record per bus kept on the device (include/mbx_limit.h); resample(pcm16, T, state, rs) -- int16 rows
upsampled to 16, 24, 32 or 48 kHz by a polyphase FIR interpolator with the caller's taps, a history record per row kept on the device
(include/mbx_resample.h); filter(pcm16, T, state, filt) -- int16 rows through a per-stream cascade of 1-4 biquads in front of the
gain, a state record per stream kept on the device (include/mbx_filter.h); bands(pcm16, bank, form) -- the rows against a caller's
bank of probes (a Bank, below), K small records per row (include/mbx_bands.h).  Sessions are not wrapped here: mbx_session_next_resample is called through _native.lib(), as every
mbx_session_* call is.
"""
import numpy as np

from . import _native
from . import bursts as _bursts
from . import keystream as _keystream
from .layout import (
    CODEC_IMBE7200X4400,
    FRAME_BYTES,
    PARMS_DTYPE,
    RECORD_DTYPE,
    RESULT_DTYPE,
    RNG_DTYPE,
    init_state,
    load_tables_blob,
    rng_default,
    rng_seeded,
)

_initialised = {}


def ensure_init(device_index, blob=None):
    """mbx_init once per (process, device) -- the native library keeps one context per device and every
    launcher uses the context of the calling thread's current device.  Returns the blob checksum."""
    device_index = int(device_index)
    if device_index not in _initialised:
        blob = blob if blob is not None else load_tables_blob()
        L = _native.lib()
        _native.check(L.mbx_init(device_index, blob, len(blob)), "mbx_init")   # also makes it the current device
        _initialised[device_index] = L.mbx_table_checksum()
    return _initialised[device_index]


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise _native.NativeLibraryError("no HIP device visible to torch; mbelib-neo_amd has no CPU fallback")
    return torch


class Bank:
    """A native bank of probes (mbx_band_bank_create, include/mbx_bands.h) on the current device: `probes` is int16 [K, 2, 160] as
    bands.tone / bands.dtmf make them, K x { c[160], s[160] }.  Immutable; usable from several streams.  Owns the native handle."""

    def __init__(self, probes):
        import ctypes

        self.handle = None
        p = np.ascontiguousarray(probes)
        if p.dtype != np.int16 or p.size % 320:
            raise ValueError("probes are int16 [K, 2, 160]")
        h = ctypes.c_void_p()
        _native.check(_native.lib().mbx_band_bank_create(ctypes.byref(h), p.ctypes.data if p.size else None, p.size // 320), "mbx_band_bank_create")
        self.handle = h
        self.probes = _native.lib().mbx_band_bank_probes(h)

    def close(self):
        if self.handle is not None:
            _native.lib().mbx_band_bank_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class BatchDecoder:
    """resident=True: the decoder owns the state between launches and uses the resident form (mbx_process_batch_resident,
    include/mbx.h): prev_mp_enhanced elided while it equals cur_mp, prev_mp fetched lazily; state_numpy() materialises the
    ABI triplets first.  PCM, results and state are bit-identical to the default."""

    def __init__(self, codec, streams, device=0, seeds=None, tables_blob=None, resident=False):
        torch = _torch()
        self.codec = int(codec)
        self.streams = int(streams)
        self.device = torch.device("cuda", int(device))
        torch.cuda.set_device(self.device)
        ensure_init(self.device.index, tables_blob)
        st = init_state(self.streams)
        rg = rng_default(self.streams) if seeds is None else rng_seeded(seeds)
        self.state = torch.from_numpy(st.view(np.uint8).reshape(-1)).to(self.device)
        self.rng = torch.from_numpy(rg.view(np.uint8).reshape(-1)).to(self.device)
        self.resident = torch.zeros(self.streams, dtype=torch.int32, device=self.device) if resident else None
        self._keystream = None   # the rows of the last keyed call

    # -- state access (host copies) --------------------------------------------------------
    def materialize(self):
        """resident decoders: write the elided prev_mp_enhanced structs out (no-op otherwise)"""
        if self.resident is not None:
            torch = _torch()
            with torch.cuda.device(self.device):
                _native.check(_native.lib().mbx_resident_materialize(self.streams, None, self.state.data_ptr(), self.resident.data_ptr(),
                                                                     torch.cuda.current_stream().cuda_stream), "mbx_resident_materialize")

    def state_numpy(self):
        self.materialize()
        return self.state.cpu().numpy().view(PARMS_DTYPE).reshape(self.streams, 3)

    def rng_numpy(self):
        return self.rng.cpu().numpy().view(RNG_DTYPE)

    def set_state(self, state, rng=None):
        torch = _torch()
        self.state.copy_(torch.from_numpy(np.ascontiguousarray(state).view(np.uint8).reshape(-1)))
        if self.resident is not None:
            self.resident.zero_()
        if rng is not None:
            self.rng.copy_(torch.from_numpy(np.ascontiguousarray(rng).view(np.uint8).reshape(-1)))

    def to_device(self, frames):
        torch = _torch()
        if isinstance(frames, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)).to(self.device)
        return frames

    def keystream_rows(self, keystream, rows):
        """The keystream of a keyed call (include/mbx_keystream.h; keystream.rows_from_bits makes it) as a device tensor: uint8
        [rows, 12], one row per batch row, torch tensor or array."""
        torch = _torch()
        if isinstance(keystream, np.ndarray) and keystream.dtype != np.uint8:
            raise ValueError("keystream must be uint8 rows of KEYSTREAM_ROW_BYTES bytes")
        d = self.to_device(keystream)
        if d.dtype != torch.uint8 or not d.is_contiguous() or d.numel() != int(rows) * _keystream.ROW_BYTES:
            raise ValueError(f"keystream must hold {int(rows)} contiguous uint8 rows of {_keystream.ROW_BYTES} bytes, one per batch row")
        return d

    # -- launches ----------------------------------------------------------------------------
    def fec(self, frames):
        """FEC stage only: wire frames -> parameter records (device tensor of uint32 [n, 4])."""
        torch = _torch()
        d_frames = self.to_device(frames)
        n = d_frames.numel() // FRAME_BYTES[self.codec]
        rec = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        L = _native.lib()
        fn = {0: L.mbx_fec_imbe7200x4400, 1: L.mbx_fec_ambe3600x2450, 2: L.mbx_fec_imbe7100x4400,
              3: L.mbx_fec_ambe3600x2450}[self.codec]   # both AMBE codecs share the FEC front end
        with torch.cuda.device(self.device):
            _native.check(fn(d_frames.data_ptr(), n, rec.data_ptr(), torch.cuda.current_stream().cuda_stream), "mbx_fec")
        return rec

    def make_outputs(self, T, want_pcm16=True, want_float=False, want_results=True, streams=None, total=None):
        """Output tensors of a launch of `streams` (default: all) x T frames, or -- total given: a ragged launch -- of `total` frames."""
        torch = _torch()
        n = (self.streams if streams is None else int(streams)) * T if total is None else int(total)
        out = {"records": torch.empty((n, 4), dtype=torch.int32, device=self.device)}
        out["pcm16"] = torch.empty((n, 160), dtype=torch.int16, device=self.device) if want_pcm16 else None
        out["pcmf"] = torch.empty((n, 160), dtype=torch.float32, device=self.device) if want_float else None
        out["results"] = torch.empty((n, 5), dtype=torch.int32, device=self.device) if want_results else None
        return out

    def compand(self, pcm16, law, out=None):
        """Companded PCM out (include/mbx_pcm8.h): mbx_pcm_compand behind a decode on the current torch stream -- the int16 rows
        [n, 160] a decode returned (a contiguous device tensor) -> uint8 [n, 160], G.711 mu-law (pcm8.LAW_ULAW) or A-law
        (pcm8.LAW_ALAW), the bytes pcm8.ulaw / pcm8.alaw give on the host.  out: a contiguous uint8 tensor of as many elements."""
        torch = _torch()
        n = _pcm16_rows(pcm16)
        if out is None:
            out = torch.empty(tuple(pcm16.shape), dtype=torch.uint8, device=pcm16.device)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != pcm16.numel() or out.device != pcm16.device:
            raise ValueError("out must be a contiguous uint8 tensor of one byte per sample on the device of pcm16")
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_pcm_compand(int(law), pcm16.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_pcm_compand")
        return out

    def mixdown(self, pcm16, plan, form=0, out=None):
        """Mix-down out (include/mbx_mixdown.h): mbx_mixdown behind a decode on the current torch stream -- the int16 rows [n, 160] a
        decode returned (a contiguous device tensor) -> the buses of `plan` (a mixdown.Plan made on that device) [plan.buses, 160]:
        int16 (mixdown.PCM16) or G.711 bytes (mixdown.ULAW, mixdown.ALAW), the values mixdown.mix gives on the host.  out: a contiguous
        tensor of that shape's element count and dtype."""
        torch = _torch()
        n = _pcm16_rows(pcm16)
        out = _bus_out(pcm16, plan, form, out)
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_mixdown(plan.handle, int(form), pcm16.data_ptr(), n, out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_mixdown")
        return out

    def levels(self, pcm16, out=None):
        """Levels out (include/mbx_levels.h): mbx_pcm_levels behind a decode on the current torch stream -- the int16 rows [n, 160] a
        decode returned (a contiguous device tensor) -> their level records as uint8 [n, 16]; ``.cpu().numpy().view(levels.LEVEL_DTYPE)``
        gives the records levels.measure gives on the host.  out: a contiguous uint8 tensor of 16 bytes per row."""
        torch = _torch()
        n = _pcm16_rows(pcm16)
        if out is None:
            out = torch.empty((n, 16), dtype=torch.uint8, device=pcm16.device)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != n * 16 or out.device != pcm16.device:
            raise ValueError("out must be a contiguous uint8 tensor of 16 bytes per row on the device of pcm16")
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_pcm_levels(pcm16.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_pcm_levels")
        return out

    def bands(self, pcm16, bank, form=0, out=None):
        """Band records (include/mbx_bands.h): mbx_pcm_bands behind a decode on the current torch stream -- the int16 rows [n, 160] a
        decode returned (a contiguous device tensor) against `bank` (a Bank) -> their records as uint8 [n, K * record_bytes], 8 bytes
        per probe for form 0 (MBX_BANDS_COMPLEX) and 4 for form 1 (MBX_BANDS_POWER); ``.cpu().numpy().view(bands.out_dtype(form))``
        gives the records bands.measure gives on the host.  out: a contiguous uint8 tensor of that size."""
        torch = _torch()
        n, form = _pcm16_rows(pcm16), int(form)
        if form not in (0, 1):
            raise ValueError("form is MBX_BANDS_COMPLEX (0) or MBX_BANDS_POWER (1)")
        per_row = bank.probes * (8 if form == 0 else 4)
        if out is None:
            out = torch.empty((n, per_row), dtype=torch.uint8, device=pcm16.device)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != n * per_row or out.device != pcm16.device:
            raise ValueError("out must be a contiguous uint8 tensor of K * record_bytes bytes per row on the device of pcm16")
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_pcm_bands(bank.handle, form, pcm16.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_pcm_bands")
        return out

    def _levels_for(self, pcm16, levels):
        """the levels tensor of a gated or held call and the rows of pcm16: what the caller got from self.levels(pcm16), or measured here"""
        torch = _torch()
        if levels is None:
            levels = self.levels(pcm16)
        n = pcm16.numel() // 160
        if levels.dtype != torch.uint8 or not levels.is_contiguous() or levels.numel() != n * 16 or levels.device != pcm16.device:
            raise ValueError("levels must be the contiguous uint8 tensor of 16 bytes per row that levels() returns for pcm16")
        return levels, n

    def mixdown_gated(self, pcm16, plan, form=0, open_peak=0, loudest_n=0, levels=None, out=None):
        """The gated mix-down (include/mbx_levels.h): mbx_mixdown_gated on the current torch stream -- the buses of `plan` summing only
        the inputs whose row's peak is at least open_peak, and with loudest_n = N > 0 only the N loudest of those, the values
        levels.mix_gated gives on the host.  levels: what self.levels(pcm16) returned; None: measured here first.  out: as for mixdown."""
        import ctypes

        from . import levels as _levels

        torch = _torch()
        levels, n = self._levels_for(pcm16, levels)
        out = _bus_out(pcm16, plan, form, out)
        if not (0 <= int(open_peak) <= 0xFFFF and 0 <= int(loudest_n) <= 0xFFFF):
            raise ValueError("open_peak and loudest_n are uint16 fields of the gate")
        gate = _levels.Gate(int(open_peak), int(loudest_n))
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_mixdown_gated(plan.handle, ctypes.addressof(gate), int(form), pcm16.data_ptr(), n, levels.data_ptr(), out.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_mixdown_gated")
        return out

    def mixdown_held(self, pcm16, plan, state, hold, form=0, levels=None, out=None):
        """The held gate (include/mbx_hold.h): mbx_mixdown_held on the current torch stream -- the buses of `plan` under `hold` (a
        hold.Hold: hysteresis, hang time, the N loudest, ramps) and `state` (a hold.GateState made for `plan`) advanced by one frame, the
        values hold.step gives on the host.  levels: what self.levels(pcm16) returned; None: measured here first.  out: as for mixdown."""
        import ctypes

        torch = _torch()
        levels, n = self._levels_for(pcm16, levels)
        out = _bus_out(pcm16, plan, form, out)
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_mixdown_held(plan.handle, ctypes.addressof(hold), state.handle, int(form), pcm16.data_ptr(), n, levels.data_ptr(),
                                                out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_mixdown_held")
        return out

    def agc(self, pcm16, T, state, agc, stream_index=None, out=None):
        """Levelled rows (include/mbx_agc.h): mbx_pcm_agc on the current torch stream -- the int16 rows [n * T, 160] a decode returned
        (a contiguous device tensor, stream-major) under `agc` (an agc.Agc) and `state` (an agc.AgcState) advanced by T frames, the
        values agc.step gives on the host.  stream_index (int32 device tensor [n]): entry i uses record stream_index[i]; without it
        record i.  out: a contiguous int16 tensor of as many elements, or pcm16 itself (in place); None: a new tensor."""
        import ctypes

        torch = _torch()
        rows, T = _pcm16_rows(pcm16), int(T)
        if T <= 0 or rows % T:
            raise ValueError("pcm16 must hold n * T rows")
        if stream_index is not None and (stream_index.dtype != torch.int32 or not stream_index.is_contiguous() or stream_index.numel() != rows // T
                                         or stream_index.device != pcm16.device):
            raise ValueError("stream_index must be a contiguous int32 tensor of one entry per stream on the device of pcm16")
        if out is None:
            out = torch.empty(tuple(pcm16.shape), dtype=torch.int16, device=pcm16.device)
        elif out.dtype != torch.int16 or not out.is_contiguous() or out.numel() != pcm16.numel() or out.device != pcm16.device:
            raise ValueError("out must be a contiguous int16 tensor of one element per sample on the device of pcm16")
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_pcm_agc(ctypes.addressof(agc), state.handle, None if stream_index is None else stream_index.data_ptr(), rows // T, T,
                                           pcm16.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_pcm_agc")
        return out

    def mixdown_sums(self, pcm16, plan, out=None):
        """The sums of mixdown (include/mbx_limit.h): mbx_mixdown_sums on the current torch stream -- the buses of `plan` as int32
        [plan.buses, 160], the sum in front of the clamp, the values limit.sums gives on the host.  out: a contiguous int32 tensor of
        that element count."""
        torch = _torch()
        n = _pcm16_rows(pcm16)
        out = _sums_out(pcm16, plan, out)
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_mixdown_sums(plan.handle, pcm16.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_mixdown_sums")
        return out

    def mixdown_gated_sums(self, pcm16, plan, open_peak=0, loudest_n=0, levels=None, out=None):
        """The sums of mixdown_gated (include/mbx_limit.h): mbx_mixdown_gated_sums on the current torch stream, the values
        limit.sums_gated gives on the host.  levels and out: as for mixdown_gated and mixdown_sums."""
        import ctypes

        from . import levels as _levels

        torch = _torch()
        levels, n = self._levels_for(pcm16, levels)
        out = _sums_out(pcm16, plan, out)
        if not (0 <= int(open_peak) <= 0xFFFF and 0 <= int(loudest_n) <= 0xFFFF):
            raise ValueError("open_peak and loudest_n are uint16 fields of the gate")
        gate = _levels.Gate(int(open_peak), int(loudest_n))
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_mixdown_gated_sums(plan.handle, ctypes.addressof(gate), pcm16.data_ptr(), n, levels.data_ptr(), out.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_mixdown_gated_sums")
        return out

    def mixdown_held_sums(self, pcm16, plan, state, hold, levels=None, out=None):
        """The sums of mixdown_held (include/mbx_limit.h): mbx_mixdown_held_sums on the current torch stream, `state` advanced by one
        frame, the values limit.sums_held gives on the host.  levels and out: as for mixdown_held and mixdown_sums."""
        import ctypes

        torch = _torch()
        levels, n = self._levels_for(pcm16, levels)
        out = _sums_out(pcm16, plan, out)
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_mixdown_held_sums(plan.handle, ctypes.addressof(hold), state.handle, pcm16.data_ptr(), n, levels.data_ptr(),
                                                     out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_mixdown_held_sums")
        return out

    def bus_limit(self, sums, T, state, limit, form=0, out=None):
        """Limited buses (include/mbx_limit.h): mbx_bus_limit on the current torch stream -- the int32 sums [n * T, 160] of a sums call
        (a contiguous device tensor, bus-major) under `limit` (a limit.Limit) and `state` (a limit.LimitState) advanced by T frames ->
        [n * T, 160] int16 (mixdown.PCM16) or G.711 bytes (mixdown.ULAW, mixdown.ALAW), the values limit.step gives on the host.
        out: a contiguous tensor of that element count and dtype."""
        import ctypes

        torch = _torch()
        T = int(T)
        if sums.dtype != torch.int32 or not sums.is_contiguous() or sums.numel() % 160:
            raise ValueError("sums must be a contiguous int32 tensor of rows of 160 samples")
        rows = sums.numel() // 160
        if T <= 0 or rows % T:
            raise ValueError("sums must hold n * T rows")
        dtype = torch.int16 if int(form) == 0 else torch.uint8
        if out is None:
            out = torch.empty((rows, 160), dtype=dtype, device=sums.device)
        elif out.dtype != dtype or not out.is_contiguous() or out.numel() != rows * 160 or out.device != sums.device:
            raise ValueError("out must be a contiguous tensor of 160 samples per row, int16 or uint8 by the form, on the device of sums")
        with torch.cuda.device(sums.device):
            rc = _native.lib().mbx_bus_limit(ctypes.addressof(limit), state.handle, rows // T, T, sums.data_ptr(), int(form), out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_bus_limit")
        return out

    def resample(self, pcm16, T, state, rs, stream_index=None, out=None):
        """Wide rows (include/mbx_resample.h): mbx_pcm_resample on the current torch stream -- the int16 rows [n * T, 160] of a decode
        or of a mix-down (a contiguous device tensor, stream-major) under `rs` (a resample.Resample) and `state` (a
        resample.ResampleState) advanced by T frames -> int16 [n * T, 160 * L], the values resample.step gives on the host.
        stream_index (int32 device tensor [n]): entry i uses record stream_index[i]; without it record i.  out: a contiguous int16
        tensor of L times as many elements, apart from pcm16; None: a new tensor."""
        import ctypes

        torch = _torch()
        rows, T, L = _pcm16_rows(pcm16), int(T), int(rs.L)
        if T <= 0 or rows % T:
            raise ValueError("pcm16 must hold n * T rows")
        if stream_index is not None and (stream_index.dtype != torch.int32 or not stream_index.is_contiguous() or stream_index.numel() != rows // T
                                         or stream_index.device != pcm16.device):
            raise ValueError("stream_index must be a contiguous int32 tensor of one entry per stream on the device of pcm16")
        if out is None:
            out = torch.empty((rows, 160 * L), dtype=torch.int16, device=pcm16.device)
        elif out.dtype != torch.int16 or not out.is_contiguous() or out.numel() != pcm16.numel() * L or out.device != pcm16.device:
            raise ValueError("out must be a contiguous int16 tensor of L elements per sample on the device of pcm16")
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_pcm_resample(ctypes.addressof(rs), state.handle, None if stream_index is None else stream_index.data_ptr(), rows // T, T,
                                                pcm16.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_pcm_resample")
        return out

    def filter(self, pcm16, T, state, filt, stream_index=None, out=None):
        """Filtered rows (include/mbx_filter.h): mbx_pcm_filter on the current torch stream -- the int16 rows [n * T, 160] a decode
        returned (a contiguous device tensor, stream-major) through the cascade `filt` (a filters.Filter) with `state` (a
        filters.FilterState) advanced by T frames, the values filters.step gives on the host.  stream_index (int32 device tensor [n]):
        entry i uses record stream_index[i]; without it record i.  out: a contiguous int16 tensor of as many elements, or pcm16 itself
        (in place); None: a new tensor."""
        import ctypes

        torch = _torch()
        rows, T = _pcm16_rows(pcm16), int(T)
        if T <= 0 or rows % T:
            raise ValueError("pcm16 must hold n * T rows")
        if stream_index is not None and (stream_index.dtype != torch.int32 or not stream_index.is_contiguous() or stream_index.numel() != rows // T
                                         or stream_index.device != pcm16.device):
            raise ValueError("stream_index must be a contiguous int32 tensor of one entry per stream on the device of pcm16")
        if out is None:
            out = torch.empty(tuple(pcm16.shape), dtype=torch.int16, device=pcm16.device)
        elif out.dtype != torch.int16 or not out.is_contiguous() or out.numel() != pcm16.numel() or out.device != pcm16.device:
            raise ValueError("out must be a contiguous int16 tensor of one element per sample on the device of pcm16")
        with torch.cuda.device(pcm16.device):
            rc = _native.lib().mbx_pcm_filter(ctypes.addressof(filt), state.handle, None if stream_index is None else stream_index.data_ptr(), rows // T, T,
                                              pcm16.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_pcm_filter")
        return out

    def decode_soft(self, soft, T, want_pcm16=True, want_float=False, want_results=True, out=None, stream_index=None, keystream=None):
        """Soft-decision frames: `soft` = torch tensor (or array) uint8 [n*T, cells, 2] = (bit, reliability), cells = 184 / 96 /
        168 / 96 for codecs 0..3, stream-major.  Runs mbx_process_batch_soft_resident on this decoder's state, resident or not.
        stream_index (int32 tensor [n]): batch row i belongs to stream stream_index[i] of this decoder (no stream twice); without
        it n = streams.  Hard decisions must be 0/1 (checked here only for host arrays).  Hard and soft calls may alternate.
        keystream (uint8 [n*T, 12]): a keyed call, mbx_process_batch_keyed -- row r is XORed onto the parameter bits of batch row r
        between FEC and parameter decode; out["records"] holds the bits after it."""
        torch = _torch()
        if isinstance(soft, np.ndarray):
            soft = _soft_array(self.codec, soft, soft.size // (SOFT_CELLS[self.codec] * 2))
            if soft.reshape(-1, 2)[:, 0].max(initial=0) > 1:
                raise ValueError("soft frames: a hard decision is not 0 or 1")
        d_soft = self.to_device(soft)
        if d_soft.dtype != torch.uint8 or not d_soft.is_contiguous():
            raise ValueError("soft frames must be a contiguous uint8 tensor")
        n = self.streams if stream_index is None else int(stream_index.numel())
        if d_soft.numel() != n * int(T) * SOFT_CELLS[self.codec] * 2:
            raise ValueError("soft must hold n*T frames of SOFT_CELLS[codec] (bit, reliability) pairs")
        if stream_index is not None:
            if stream_index.dtype != torch.int32 or stream_index.device != self.device:
                raise ValueError("stream_index must be an int32 tensor on the decoder's device")
            if n and (int(torch.unique(stream_index).numel()) != n or int(stream_index.min()) < 0 or int(stream_index.max()) >= self.streams):
                raise ValueError("stream_index: out of range, or a stream listed twice (two rows would race on one state)")
        if out is None:
            out = self.make_outputs(T, want_pcm16, want_float, want_results, streams=n)

        def ptr(t):
            return t.data_ptr() if t is not None else None

        d_key = self.keystream_rows(keystream, n * int(T)) if keystream is not None else None
        with torch.cuda.device(self.device):
            if d_key is not None:
                rc = _native.lib().mbx_process_batch_keyed(
                    self.codec, n, int(T), ptr(stream_index), None, d_soft.data_ptr(), d_key.data_ptr(), self.state.data_ptr(),
                    ptr(self.resident), self.rng.data_ptr(), ptr(out["pcm16"]), ptr(out["pcmf"]), ptr(out["results"]),
                    out["records"].data_ptr(), torch.cuda.current_stream().cuda_stream,
                )
                self._keystream = d_key   # the launch is asynchronous: the decoder holds the uploaded rows until its next keyed call
            else:
                rc = _native.lib().mbx_process_batch_soft_resident(
                    self.codec, n, int(T), ptr(stream_index), d_soft.data_ptr(), self.state.data_ptr(), ptr(self.resident),
                    self.rng.data_ptr(), ptr(out["pcm16"]), ptr(out["pcmf"]), ptr(out["results"]), out["records"].data_ptr(),
                    torch.cuda.current_stream().cuda_stream,
                )
        _native.check(rc, "mbx_process_batch_keyed" if d_key is not None else "mbx_process_batch_soft_resident")
        return out

    def decode_bursts(self, schedule, bursts, soft=False, want_pcm16=True, want_float=False, want_results=True, out=None, stream_index=None,
                      burst_stride=None):
        """Received bursts instead of frames: `schedule` (bursts.BurstSchedule, of this decoder's codec) says where the channel bits of
        the F frames of a burst sit; burst row i carries the next F frames of stream i (stream_index[i]).  One mbx_process_bursts /
        _soft call: the gather on the device, then the step decode(frames, T=F) / decode_soft run, on this decoder's state, resident
        or not.  bursts: uint8 tensor or array in the schedule's form -- hard: n bursts of burst_stride bytes (default
        schedule.burst_bytes); soft=True: [n, schedule.soft_cells, 2] (bit or dibit, reliability), of an LLR schedule [n, burst_bits]
        int16 / int8.  A host array is checked with
        mbx_burst_validate; a device tensor is the caller's to check.  Returns the dict of decode at T = F."""
        torch = _torch()
        if schedule.codec != self.codec:
            raise ValueError("the schedule is of another codec than the decoder")
        stride = schedule.burst_bytes if burst_stride is None else int(burst_stride)
        bursts = _bursts.as_bytes(schedule, bursts, soft)
        if isinstance(bursts, np.ndarray):
            per = schedule.soft_bytes if soft else stride
            if per > 0 and bursts.size % per == 0 and _native.lib().mbx_burst_validate(schedule.handle, bursts.ctypes.data, stride, bursts.size // per, int(soft)) == -2:
                raise ValueError("soft bursts: a hard decision is not 0 or 1 (a dibit not 0 .. 3)" if soft else "bursts: a bit byte is not 0 or 1, or a dibit byte not 0 .. 3")
        d_bursts = self.to_device(bursts)
        if d_bursts.dtype != torch.uint8 or not d_bursts.is_contiguous():
            raise ValueError("bursts must be a contiguous uint8 tensor")
        n = self.streams if stream_index is None else int(stream_index.numel())
        if d_bursts.numel() != n * (schedule.soft_bytes if soft else stride):
            raise ValueError("bursts must hold one burst per batch row")
        if stream_index is not None:
            if stream_index.dtype != torch.int32 or stream_index.device != self.device:
                raise ValueError("stream_index must be an int32 tensor on the decoder's device")
            if n and (int(torch.unique(stream_index).numel()) != n or int(stream_index.min()) < 0 or int(stream_index.max()) >= self.streams):
                raise ValueError("stream_index: out of range, or a stream listed twice (two rows would race on one state)")
        if out is None:
            out = self.make_outputs(schedule.frames_per_burst, want_pcm16, want_float, want_results, streams=n)

        def ptr(t):
            return t.data_ptr() if t is not None else None

        L = _native.lib()
        tail = (self.state.data_ptr(), ptr(self.resident), self.rng.data_ptr(), ptr(out["pcm16"]), ptr(out["pcmf"]), ptr(out["results"]),
                out["records"].data_ptr(), None)
        with torch.cuda.device(self.device):
            tail = tail[:-1] + (torch.cuda.current_stream().cuda_stream,)
            if soft:
                rc = L.mbx_process_bursts_soft(schedule.handle, n, ptr(stream_index), d_bursts.data_ptr(), *tail)
            else:
                rc = L.mbx_process_bursts(schedule.handle, n, ptr(stream_index), d_bursts.data_ptr(), stride, *tail)
        _native.check(rc, "mbx_process_bursts")
        return out

    def decode_burst_groups(self, groups, soft=False, want_pcm16=True, want_float=False, want_results=True, out=None):
        """Burst groups (bursts.BurstGroup, up to bursts.MAX_GROUPS, all hard or all soft): the bursts of several schedules, of any
        codecs, decoded by ONE mbx_process_burst_groups call on this decoder's state pool, resident or not, whatever the decoder's own
        codec is -- one gather launch over all groups, then one mixed ragged step.  Rows run group after group, inside a group stream
        after stream, burst after burst, frame after frame.  Host bursts are checked with mbx_burst_validate and uploaded, device
        tensors are the caller's to check; the slots the groups name are checked here (in range, none twice).  The codec of a slot
        stays what it was in its earlier calls: that is the caller's to keep.  Returns the dict of decode plus "row_of_group"
        (int32 host array, len(groups) + 1)."""
        torch = _torch()
        groups = list(groups)
        if len(groups) > _bursts.MAX_GROUPS:
            raise ValueError("at most MAX_GROUPS groups in one call")
        row_of_group = _bursts.group_rows(groups)
        slots = np.concatenate([g.slots() for g in groups]) if groups else np.zeros(0, dtype=np.int32)
        if slots.size and (np.unique(slots).size != slots.size or slots.min() < 0 or slots.max() >= self.streams):
            raise ValueError("stream_index: out of range, or a slot named twice (two rows would race on one state)")
        L = _native.lib()
        keep, pointers = [], []
        for g in groups:
            s = g.schedule
            b = _bursts.as_bytes(s, g.bursts, soft)
            if not isinstance(b, np.ndarray) and (b.dtype != torch.uint8 or not b.is_contiguous()):
                raise ValueError("bursts must be a contiguous uint8 tensor")
            # of the last hard burst the schedule's bytes are read, not its whole stride
            per = s.soft_bytes if soft else g.burst_stride
            need = (g.n_bursts - 1) * per + (per if soft else s.burst_bytes) if g.n_bursts else 0
            if (b.size if isinstance(b, np.ndarray) else b.numel()) < need:
                raise ValueError("bursts must hold n_streams * bursts_per_stream bursts")
            if isinstance(b, np.ndarray) and g.n_bursts and L.mbx_burst_validate(s.handle, b.ctypes.data, g.burst_stride, g.n_bursts, int(soft)) == -2:
                raise ValueError("burst groups: a bit byte, dibit or hard decision above its range")
            d_b = self.to_device(b)
            idx = g.stream_index
            if idx is not None and not isinstance(idx, torch.Tensor):
                idx = torch.from_numpy(g.slots()).to(self.device)
            if idx is not None and (idx.dtype != torch.int32 or idx.device != self.device or idx.numel() != g.n_streams):
                raise ValueError("stream_index must be an int32 tensor of n_streams slots on the decoder's device")
            keep.append((d_b, idx))
            pointers.append((d_b.data_ptr() if d_b.numel() else 0, idx.data_ptr() if idx is not None and idx.numel() else 0))
        if out is None:
            out = self.make_outputs(0, want_pcm16, want_float, want_results, total=int(row_of_group[-1]))
        out["row_of_group"] = row_of_group

        def ptr(t):
            return t.data_ptr() if t is not None else None

        arr = _bursts.group_structs(groups, pointers)
        with torch.cuda.device(self.device):
            rc = L.mbx_process_burst_groups(arr, len(groups), int(soft), self.state.data_ptr(), ptr(self.resident), self.rng.data_ptr(),
                                            ptr(out["pcm16"]), ptr(out["pcmf"]), ptr(out["results"]), out["records"].data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_process_burst_groups")
        out["_inputs"] = keep   # the launch is asynchronous: the uploaded bursts live as long as the outputs
        return out

    def decode_ragged(self, frames, counts, soft=False, want_pcm16=True, want_float=False, want_results=True, out=None, stream_index=None,
                      codec=None, keystream=None):
        """A frame count per stream: row i of the batch brings counts[i] >= 0 frames (host sequence or array), its rows of `frames`
        and of every output are offsets[i] .. offsets[i + 1] - 1 with offsets = [0, cumsum(counts)], in time order.  One
        mbx_process_batch_ragged / _soft_ragged call on this decoder's state, resident or not; soft=True: `frames` holds
        mbe_soft_bit cells as in decode_soft.  stream_index (int32 tensor [n]): row i belongs to stream stream_index[i] (no stream
        twice); without it n = streams.  A stream with count 0 keeps its state.  Returns the dict of decode plus "offsets" (int32
        device tensor [n + 1]).
        codec (array of n MBX_CODEC_* values): a MIXED batch, row i of codec[i], decoded by one mbx_process_batch_mixed /
        _soft_mixed call whatever the decoder's own codec is; `frames` then holds rows of ONE size, MIXED_ROW_BYTES bytes
        (soft: MIXED_ROW_CELLS cells), as pack_mixed_rows makes them from each stream's own frames -- or is the list of per-stream
        arrays itself.  The codec of a stream stays what it was in the stream's earlier calls: that is the caller's to keep.
        keystream (uint8 [sum(counts), 12]): a keyed call, mbx_process_batch_ragged_keyed -- row r onto the parameter bits of
        batch row r, whatever its codec."""
        counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
        n = self.streams if stream_index is None else int(stream_index.numel())
        if counts.size != n or (n and counts.min() < 0):
            raise ValueError("counts must hold one frame count >= 0 per batch row")
        total = int(counts.sum())
        if total > 0x7FFFFFFF:
            raise ValueError("more than 2^31-1 frames in one launch")
        mixed = codec is not None
        if mixed:   # (everything the host can check, before torch or the library is touched)
            codec = mixed_codecs(codec, n)
            if isinstance(frames, (list, tuple)):
                frames = pack_mixed_rows(codec, counts, frames, soft)
            row_bytes = MIXED_ROW_CELLS * 2 if soft else MIXED_ROW_BYTES
            if isinstance(frames, np.ndarray) and (frames.dtype != np.uint8 or frames.size != total * row_bytes):
                raise ValueError(f"frames must hold sum(counts) = {total} uint8 rows of {row_bytes} bytes")
        else:
            row_bytes = SOFT_CELLS[self.codec] * 2 if soft else FRAME_BYTES[self.codec]
        torch = _torch()
        if soft and isinstance(frames, np.ndarray):
            if not mixed:
                frames = _soft_array(self.codec, frames, total)
            if frames.reshape(-1, 2)[:, 0].max(initial=0) > 1:
                raise ValueError("soft frames: a hard decision is not 0 or 1")
        d_frames = self.to_device(frames)
        if d_frames.dtype != torch.uint8 or not d_frames.is_contiguous():
            raise ValueError("frames must be a contiguous uint8 tensor")
        if d_frames.numel() != total * row_bytes:
            raise ValueError("frames must hold sum(counts) frames")
        if stream_index is not None:
            if stream_index.dtype != torch.int32 or stream_index.device != self.device:
                raise ValueError("stream_index must be an int32 tensor on the decoder's device")
            if n and (int(torch.unique(stream_index).numel()) != n or int(stream_index.min()) < 0 or int(stream_index.max()) >= self.streams):
                raise ValueError("stream_index: out of range, or a stream listed twice (two rows would race on one state)")
        offsets = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(counts, out=offsets[1:])
        d_offsets = torch.from_numpy(offsets).to(self.device)
        if out is None:
            out = self.make_outputs(0, want_pcm16, want_float, want_results, total=total)
        out["offsets"] = d_offsets

        def ptr(t):
            return t.data_ptr() if t is not None else None

        L = _native.lib()
        tail = (d_offsets.data_ptr(), total, ptr(stream_index), d_frames.data_ptr(), self.state.data_ptr(), ptr(self.resident),
                self.rng.data_ptr(), ptr(out["pcm16"]), ptr(out["pcmf"]), ptr(out["results"]), out["records"].data_ptr())
        d_key = self.keystream_rows(keystream, total) if keystream is not None else None
        with torch.cuda.device(self.device):
            if d_key is not None:
                d_codec = torch.from_numpy(codec).to(self.device) if mixed else None
                rc = L.mbx_process_batch_ragged_keyed(self.codec, ptr(d_codec), n, d_offsets.data_ptr(), total, ptr(stream_index),
                                                      None if soft else d_frames.data_ptr(), d_frames.data_ptr() if soft else None,
                                                      d_key.data_ptr(), *tail[4:], torch.cuda.current_stream().cuda_stream)
                self._keystream = d_key   # the launch is asynchronous: the decoder holds the uploaded rows until its next keyed call
                _native.check(rc, "mbx_process_batch_ragged_keyed")
                return out
            if mixed:
                d_codec = torch.from_numpy(codec).to(self.device)
                rc = (L.mbx_process_batch_soft_mixed if soft else L.mbx_process_batch_mixed)(
                    n, d_codec.data_ptr(), *tail, torch.cuda.current_stream().cuda_stream)
            else:
                rc = (L.mbx_process_batch_soft_ragged if soft else L.mbx_process_batch_ragged)(
                    self.codec, n, *tail, torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_process_batch_mixed" if mixed else "mbx_process_batch_ragged")
        return out

    def decode(self, frames, T, want_pcm16=True, want_float=False, want_results=True, out=None, staged=False, keystream=None):
        """S x T frames, stream-major (stream s, frame t at index s*T + t).  Asynchronous on the
        current torch stream; returns device tensors.
        staged=True: the stages as separate calls (mbx_fec_* then mbx_process_records) instead of mbx_process_batch -- the
        same results by contract; the IMBE codecs at T = 1 take one fused launch in mbx_process_batch and the FEC /
        expansion / stream launches here (tests compare the two).
        keystream (uint8 [streams*T, 12]): a keyed call, mbx_process_batch_keyed -- row r is XORed onto the parameter bits of
        batch row r between FEC and parameter decode (staged=True: mbx_apply_keystream between the two calls); out["records"]
        holds the bits after it."""
        torch = _torch()
        d_frames = self.to_device(frames)
        n = self.streams * int(T)
        if d_frames.numel() != n * FRAME_BYTES[self.codec]:
            raise ValueError("frames must hold streams*T wire frames")
        if out is None:
            out = self.make_outputs(T, want_pcm16, want_float, want_results)

        def ptr(t):
            return t.data_ptr() if t is not None else None

        d_key = self.keystream_rows(keystream, n) if keystream is not None else None
        if d_key is not None:
            self._keystream = d_key   # the launch is asynchronous: the decoder holds the uploaded rows until its next keyed call
        with torch.cuda.device(self.device):   # the launcher works on the current device's context
            if d_key is not None and not staged:
                rc = _native.lib().mbx_process_batch_keyed(
                    self.codec, self.streams, int(T), None, d_frames.data_ptr(), None, d_key.data_ptr(), self.state.data_ptr(),
                    ptr(self.resident), self.rng.data_ptr(), ptr(out["pcm16"]), ptr(out["pcmf"]), ptr(out["results"]),
                    out["records"].data_ptr(), torch.cuda.current_stream().cuda_stream,
                )
            elif staged:
                if self.resident is not None:
                    raise ValueError("staged decoding is for the ABI-triplet form")
                L = _native.lib()
                strm = torch.cuda.current_stream().cuda_stream
                fn = {0: L.mbx_fec_imbe7200x4400, 1: L.mbx_fec_ambe3600x2450, 2: L.mbx_fec_imbe7100x4400, 3: L.mbx_fec_ambe3600x2450}[self.codec]
                _native.check(fn(d_frames.data_ptr(), n, out["records"].data_ptr(), strm), "mbx_fec")
                if d_key is not None:
                    _native.check(L.mbx_apply_keystream(self.codec, out["records"].data_ptr(), n, d_key.data_ptr(), strm), "mbx_apply_keystream")
                rc = L.mbx_process_records(0 if self.codec == 2 else self.codec, self.streams, int(T), out["records"].data_ptr(),
                                           self.state.data_ptr(), self.rng.data_ptr(), ptr(out["pcm16"]), ptr(out["pcmf"]),
                                           ptr(out["results"]), strm)
            elif self.resident is not None:
                rc = _native.lib().mbx_process_batch_resident(
                    self.codec, self.streams, int(T), None, d_frames.data_ptr(), self.state.data_ptr(), self.resident.data_ptr(),
                    self.rng.data_ptr(), ptr(out["pcm16"]), ptr(out["pcmf"]), ptr(out["results"]), out["records"].data_ptr(),
                    torch.cuda.current_stream().cuda_stream,
                )
            else:
                rc = _native.lib().mbx_process_batch(
                    self.codec, self.streams, int(T), d_frames.data_ptr(), self.state.data_ptr(), self.rng.data_ptr(),
                    ptr(out["pcm16"]), ptr(out["pcmf"]), ptr(out["results"]), out["records"].data_ptr(),
                    torch.cuda.current_stream().cuda_stream,
                )
        _native.check(rc, "mbx_process_batch")
        return out


def results_numpy(t):
    return t.cpu().numpy().view(RESULT_DTYPE).reshape(-1)


RESULT_HIST_FIELDS = ("frames", "soft_input", "c0_valid", "c4_valid", "flag3", "tone", "erasure", "repeat", "mute", "c0_errors",
                      "protected_errors", "c4_errors", "total_errors", "frames_with_errors")


def result_histogram(results, stream=None):
    """mbx_result_histogram over a device tensor of mbe_process_result (as the decoders return them): the per-batch tally of flags
    and error counts, formed on the device (include/mbx.h: mbx_result_hist).  Returns a dict of Python ints."""
    torch = _torch()
    L = _native.lib()
    n = results.numel() * results.element_size() // RESULT_DTYPE.itemsize
    hist = torch.zeros(len(RESULT_HIST_FIELDS), dtype=torch.int64, device=results.device)
    _native.check(L.mbx_result_histogram(results.data_ptr(), n, hist.data_ptr(), stream if stream is not None else torch.cuda.current_stream().cuda_stream),
                  "mbx_result_histogram")
    return dict(zip(RESULT_HIST_FIELDS, (int(v) for v in hist.cpu().tolist())))


def records_numpy(t):
    return t.cpu().numpy().view(RECORD_DTYPE).reshape(-1)


def synthesize_speech(cur, prev, rng, device=0, want_pcm16=False):
    """mbe_synthesizeSpeechf for S (cur, prev) pairs given as numpy PARMS arrays; returns
    (pcmf [S,160], cur', prev', rng', pcm16 or None).  Host buffers in, host buffers out."""
    ensure_init(device)
    cur = np.ascontiguousarray(cur).copy()
    prev = np.ascontiguousarray(prev).copy()
    rng = np.ascontiguousarray(rng).copy()
    S = cur.shape[0]
    pcmf = np.empty((S, 160), dtype=np.float32)
    pcm16 = np.empty((S, 160), dtype=np.int16) if want_pcm16 else None
    rc = _native.lib().mbx_synthesize_speech_host(
        S, cur.ctypes.data, prev.ctypes.data, rng.ctypes.data, pcmf.ctypes.data,
        pcm16.ctypes.data if pcm16 is not None else None,
    )
    _native.check(rc, "mbx_synthesize_speech_host")
    return pcmf, cur, prev, rng, pcm16


def floattoshort(pcmf, device=0):
    """mbe_floattoshort over [n,160] float frames (host in/out)."""
    ensure_init(device)
    pcmf = np.ascontiguousarray(pcmf, dtype=np.float32)
    out = np.empty(pcmf.shape, dtype=np.int16)
    _native.check(_native.lib().mbx_floattoshort_host(pcmf.ctypes.data, out.ctypes.data, pcmf.shape[0]), "mbx_floattoshort_host")
    return out


def process_batch_host(codec, S, T, frames, state, rng, device=0):
    """Whole pipeline on host buffers (numpy in, numpy out): returns dict."""
    ensure_init(device)
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    state = np.ascontiguousarray(state).copy()
    rng = np.ascontiguousarray(rng).copy()
    n = S * T
    pcm16 = np.empty((n, 160), dtype=np.int16)
    pcmf = np.empty((n, 160), dtype=np.float32)
    results = np.empty(n, dtype=RESULT_DTYPE)
    records = np.empty(n, dtype=RECORD_DTYPE)
    rc = _native.lib().mbx_process_batch_host(
        codec, S, T, frames.ctypes.data, state.ctypes.data, rng.ctypes.data, pcm16.ctypes.data, pcmf.ctypes.data,
        results.ctypes.data, records.ctypes.data,
    )
    _native.check(rc, "mbx_process_batch_host")
    return {"pcm16": pcm16, "pcmf": pcmf, "results": results, "records": records, "state": state, "rng": rng}


# ---- soft-decision front end (mbe_soft_bit arrays: uint8 [..., 2] = (bit, reliability)) ------------
SOFT_CELLS = {0: 184, 1: 96, 2: 168, 3: 96}


# a mixed batch (decode_ragged(codec=array)): rows of one size for all codecs, the largest codec's
MIXED_ROW_BYTES, MIXED_ROW_CELLS = 18, 184


def mixed_codecs(codec, n):
    """the per-row codec array of a mixed batch as the uint8 array the library takes; ValueError unless n values in 0..3"""
    codec = np.asarray(codec)
    if codec.ndim != 1 or codec.size != n:
        raise ValueError(f"codec must hold one MBX_CODEC_* value per batch row ({n})")
    if codec.dtype.kind not in "iu" or (n and (codec.min() < 0 or codec.max() > 3)):
        raise ValueError("codec: every value must be one of 0 (IMBE 7200x4400), 1 (AMBE 3600x2450), 2 (IMBE 7100x4400), 3 (AMBE 3600x2400)")
    return np.ascontiguousarray(codec, dtype=np.uint8)


def pack_mixed_rows(codec, counts, frames, soft=False):
    """The rows of a mixed batch from each stream's own frames: frames[i] holds counts[i] frames of codec[i] -- FRAME_BYTES[codec[i]]
    bytes each, or soft: SOFT_CELLS[codec[i]] (bit, reliability) pairs -- and lands, frame by frame, at the FRONT of rows of
    MIXED_ROW_BYTES bytes (soft: MIXED_ROW_CELLS pairs); the rest of a row is zero and ignored.  Returns uint8 [sum(counts), 18]
    (soft: [sum(counts), 184, 2]).  Host only."""
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    codec = mixed_codecs(codec, counts.size)
    if len(frames) != counts.size:
        raise ValueError("frames must hold one array per batch row")
    width = MIXED_ROW_CELLS * 2 if soft else MIXED_ROW_BYTES
    rows = np.zeros((int(counts.sum()), width), dtype=np.uint8)
    at = 0
    for i, (c, k) in enumerate(zip(codec.tolist(), counts.tolist())):
        own = SOFT_CELLS[c] * 2 if soft else FRAME_BYTES[c]
        f = np.ascontiguousarray(frames[i], dtype=np.uint8)
        if f.size != k * own:
            raise ValueError(f"frames[{i}] must hold counts[{i}] = {k} frames of {own} bytes (codec {c})")
        rows[at:at + k, :own] = f.reshape(k, own)
        at += k
    return rows.reshape(-1, MIXED_ROW_CELLS, 2) if soft else rows


def _pcm16_rows(pcm16):
    """the rows of the int16 tensor a decode returned"""
    if pcm16.dtype != _torch().int16 or not pcm16.is_contiguous() or pcm16.numel() % 160:
        raise ValueError("pcm16 must be a contiguous int16 tensor of rows of 160 samples")
    return pcm16.numel() // 160


def _bus_out(pcm16, plan, form, out):
    """the bus rows of `plan` in `form` on the device of pcm16: a new tensor, or the caller's, checked"""
    torch = _torch()
    dtype = torch.int16 if int(form) == 0 else torch.uint8
    if out is None:
        return torch.empty((plan.buses, 160), dtype=dtype, device=pcm16.device)
    if out.dtype != dtype or not out.is_contiguous() or out.numel() != plan.buses * 160 or out.device != pcm16.device:
        raise ValueError("out must be a contiguous tensor of 160 samples per bus, int16 or uint8 by the form, on the device of pcm16")
    return out


def _sums_out(pcm16, plan, out):
    """the int32 sums of the buses of `plan` on the device of pcm16: a new tensor, or the caller's, checked"""
    torch = _torch()
    if out is None:
        return torch.empty((plan.buses, 160), dtype=torch.int32, device=pcm16.device)
    if out.dtype != torch.int32 or not out.is_contiguous() or out.numel() != plan.buses * 160 or out.device != pcm16.device:
        raise ValueError("out must be a contiguous int32 tensor of 160 sums per bus on the device of pcm16")
    return out


def _soft_array(codec, soft, n):
    soft = np.ascontiguousarray(soft, dtype=np.uint8)
    if soft.size != n * SOFT_CELLS[codec] * 2:
        raise ValueError(f"expected {n} soft frames of {SOFT_CELLS[codec]} (bit, reliability) pairs")
    return soft


def fec_soft_host(codec, soft, device=0):
    """mbe_decode*SoftFrame for a batch: soft [n, 184|96, 2] uint8 -> parameter records."""
    ensure_init(device)
    soft = np.ascontiguousarray(soft, dtype=np.uint8)
    n = soft.size // (SOFT_CELLS[codec] * 2)
    soft = _soft_array(codec, soft, n)
    records = np.empty(n, dtype=RECORD_DTYPE)
    _native.check(_native.lib().mbx_fec_soft_host(codec, soft.ctypes.data, n, records.ctypes.data), "mbx_fec_soft_host")
    return records


def process_batch_soft_host(codec, S, T, soft, state, rng, device=0):
    """mbe_process*SoftFramef for S streams x T frames on host buffers."""
    ensure_init(device)
    n = S * T
    soft = _soft_array(codec, soft, n)
    state = np.ascontiguousarray(state).copy()
    rng = np.ascontiguousarray(rng).copy()
    pcm16 = np.empty((n, 160), dtype=np.int16)
    pcmf = np.empty((n, 160), dtype=np.float32)
    results = np.empty(n, dtype=RESULT_DTYPE)
    records = np.empty(n, dtype=RECORD_DTYPE)
    rc = _native.lib().mbx_process_batch_soft_host(
        codec, S, T, soft.ctypes.data, state.ctypes.data, rng.ctypes.data, pcm16.ctypes.data, pcmf.ctypes.data,
        results.ctypes.data, records.ctypes.data,
    )
    _native.check(rc, "mbx_process_batch_soft_host")
    return {"pcm16": pcm16, "pcmf": pcmf, "results": results, "records": records, "state": state, "rng": rng}


def ecc_soft_words_host(kind, soft, device=0):
    """mbe_golay2312Soft (kind 0, soft [n, 23, 2]) / mbe_hamming1511Soft (kind 1, soft [n, 15, 2]) /
    mbe_7100x4400hamming1511Soft (kind 2):
    returns (corrected words, return values)."""
    ensure_init(device)
    width = 23 if kind == 0 else 15
    soft = np.ascontiguousarray(soft, dtype=np.uint8)
    n = soft.size // (width * 2)
    out = np.empty(n, dtype=np.uint32)
    errs = np.empty(n, dtype=np.int32)
    rc = _native.lib().mbx_ecc_soft_words_host(kind, soft.ctypes.data, n, out.ctypes.data, errs.ctypes.data)
    _native.check(rc, "mbx_ecc_soft_words_host")
    return out, errs


def soft_from_llr(llr, out=None):
    """mbx_soft_from_llr on the current torch stream: an int16 or int8 device tensor of LLRs, any shape -> uint8 [..., 2] cells
    (bit, reliability), the bytes soft_bits_from_llr gives on the host.  For callers that hold frame-shaped LLR arrays and go on
    to decode_soft; bursts of LLRs need no such call (bursts.FORM_LLR16 / FORM_LLR8)."""
    torch = _torch()
    if llr.dtype not in (torch.int16, torch.int8) or not llr.is_contiguous():
        raise ValueError("llr must be a contiguous int16 or int8 tensor")
    if out is None:
        out = torch.empty(tuple(llr.shape) + (2,), dtype=torch.uint8, device=llr.device)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != 2 * llr.numel():
        raise ValueError("out must be a contiguous uint8 tensor of two bytes per LLR")
    with torch.cuda.device(llr.device):
        rc = _native.lib().mbx_soft_from_llr(llr.data_ptr(), llr.element_size(), llr.numel(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "mbx_soft_from_llr")
    return out


def soft_bits_from_llr(llr):
    llr = np.ascontiguousarray(llr, dtype=np.int16)
    soft = np.empty(llr.shape + (2,), dtype=np.uint8)
    _native.check(_native.lib().mbx_soft_bits_from_llr(llr.ctypes.data, soft.ctypes.data, llr.size), "mbx_soft_bits_from_llr")
    return soft


def records_from_bits(bits, total_errors=None, c0_errors=None, flags=0):
    """Parameter records from bit arrays [n, 88|49] (0/1) -- the mbe_process*Data entry of the batch API.
    total_errors goes into the protected-error field unless c0_errors is given (then flags should carry
    MBE_PROCESS_FLAG_C0_VALID = 2)."""
    bits = np.asarray(bits, dtype=np.uint8)
    n, nb = bits.shape
    padded = np.zeros((n, 96), dtype=np.uint8)
    padded[:, :nb] = bits
    words = np.packbits(padded, axis=1).reshape(n, 3, 4)
    rec = np.zeros(n, dtype=RECORD_DTYPE)
    rec["w"][:, :3] = (words[:, :, 0].astype(np.uint32) << 24) | (words[:, :, 1].astype(np.uint32) << 16) | (
        words[:, :, 2].astype(np.uint32) << 8) | words[:, :, 3].astype(np.uint32)
    tot = np.zeros(n, dtype=np.uint32) if total_errors is None else np.asarray(total_errors, dtype=np.uint32)
    c0 = np.zeros(n, dtype=np.uint32) if c0_errors is None else np.asarray(c0_errors, dtype=np.uint32)
    rec["w"][:, 3] = c0 | ((tot - c0) << 8) | (np.uint32(flags) << 24)
    return rec


def process_records_host(codec, S, T, records, state, rng, device=0):
    """mbx_process_records on host buffers: records [S*T] stream-major; returns dict like process_batch_host."""
    torch = _torch()
    ensure_init(device)
    dev = torch.device("cuda", int(device))
    n = S * T
    d_rec = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1)).to(dev)
    d_state = torch.from_numpy(np.ascontiguousarray(state).view(np.uint8).reshape(-1).copy()).to(dev)
    d_rng = torch.from_numpy(np.ascontiguousarray(rng).view(np.uint8).reshape(-1).copy()).to(dev)
    pcm16 = torch.empty((n, 160), dtype=torch.int16, device=dev)
    pcmf = torch.empty((n, 160), dtype=torch.float32, device=dev)
    results = torch.empty((n, 5), dtype=torch.int32, device=dev)
    rc = _native.lib().mbx_process_records(codec, S, T, d_rec.data_ptr(), d_state.data_ptr(), d_rng.data_ptr(), pcm16.data_ptr(),
                                           pcmf.data_ptr(), results.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "mbx_process_records")
    torch.cuda.synchronize()
    return {
        "pcm16": pcm16.cpu().numpy(), "pcmf": pcmf.cpu().numpy(), "results": results_numpy(results),
        "state": d_state.cpu().numpy().view(PARMS_DTYPE).reshape(S, 3), "rng": d_rng.cpu().numpy().view(RNG_DTYPE),
    }
