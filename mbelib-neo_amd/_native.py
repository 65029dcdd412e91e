"""ctypes binding of the C-ABI HIP launcher (include/mbx.h, include/mbx_burst.h, include/mbx_llr.h,
include/mbx_burst_groups.h, include/mbx_keystream.h, include/mbx_pcm8.h, include/mbx_mixdown.h, include/mbx_levels.h, include/mbx_hold.h, include/mbx_agc.h, include/mbx_limit.h, include/mbx_resample.h, include/mbx_filter.h, include/mbx_bands.h, include/mbx_vote.h).  Fails loudly when the library
is missing or cannot be initialised: there is no Python/CPU stand-in."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libmbx_hip.so"


class NativeLibraryError(RuntimeError):
    pass


def library_path():
    """The product library, or the build named by MBX_HIP_LIBRARY: for tools/ the development builds (libmbx_hip_ablate.so, which
    additionally exports mbx_debug_set_ablation), for one test the fault-injection build (libmbx_hip_testing.so: mbx_testing_set_front_skip)."""
    return os.environ.get("MBX_HIP_LIBRARY") or os.path.join(_HERE, _LIB_NAME)


_lib = None

_vp = C.c_void_p
_sz = C.c_size_t
_SIGNATURES = {
    "mbx_init": (C.c_int, [C.c_int, _vp, _sz]),
    "mbx_shutdown": (None, []),
    "mbx_reserve": (C.c_int, [_sz]),
    "mbx_reserve_stream": (C.c_int, [_vp, _sz]),
    "mbx_uses_expand_launch": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "mbx_release_stream": (C.c_int, [_vp]),
    "mbx_workspace_bytes": (_sz, [_sz]),
    "mbx_device_ready": (C.c_int, [C.c_int]),
    "mbx_set_stream_order": (C.c_int, [C.c_int]),
    "mbx_set_tone_synthesis": (C.c_int, [C.c_int]),
    "mbx_table_checksum": (C.c_uint32, []),
    "mbx_last_error": (C.c_char_p, []),
    "mbx_comm_unique_id": (C.c_int, [_vp]),
    "mbx_comm_init": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int]),
    "mbx_comm_destroy": (C.c_int, [_vp]),
    "mbx_comm_agree": (C.c_int, [_vp, C.c_uint32, _vp, _vp]),
    "mbx_init_broadcast": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _sz, _vp, _vp]),
    "mbx_pack_imbe7200x4400": (C.c_int, [_vp, _sz, _vp]),
    "mbx_pack_ambe3600x2450": (C.c_int, [_vp, _sz, _vp]),
    "mbx_pack_cells": (C.c_int, [C.c_int, _vp, _sz, _vp, _vp, _vp]),
    "mbx_wire_bit_of_cell": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "mbx_wire_permutation": (C.c_int, [C.c_int, _vp, _vp, C.c_int, _vp]),
    "mbx_unpack_records": (None, [_vp, _sz, C.c_int, _vp, _vp]),
    "mbx_fec_imbe7200x4400": (C.c_int, [_vp, _sz, _vp, _vp]),
    "mbx_fec_ambe3600x2450": (C.c_int, [_vp, _sz, _vp, _vp]),
    "mbx_process_records": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_records_ws": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mbx_process_batch_ws": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mbx_expand_records": (C.c_int, [C.c_int, _vp, _sz, _vp]),
    "mbx_stream_expanded": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_stage_in": (C.c_int, [_vp, _vp, _sz, _vp]),
    "mbx_frame_server_start": (C.c_int, [_vp, C.c_uint, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_frame": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    "mbx_process_frame_shadow": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_int, _vp, _vp]),
    "mbx_process_batch_indexed": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_batch_resident": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_resident_materialize": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp]),
    "mbx_expand_records_ws": (C.c_int, [C.c_int, _vp, _sz, _vp, _sz, _vp]),
    "mbx_stream_expanded_ws": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mbx_stream_expanded_resident": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_fec_stage": (C.c_int, [C.c_int, C.c_int, _vp, _sz, _vp, _vp, _vp]),
    "mbx_decode_parms": (C.c_int, [C.c_int, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mbx_synthesize_speech": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_floattoshort": (C.c_int, [_vp, _vp, _sz, _vp]),
    "mbx_result_histogram": (C.c_int, [_vp, _sz, _vp, _vp]),
    "mbx_spectral_amp_enhance": (C.c_int, [C.c_int, _vp, _vp]),
    "mbx_adaptive_smoothing": (C.c_int, [C.c_int, _vp, _vp, _vp]),
    "mbx_comfort_noise": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp]),
    "mbx_ecc_words": (C.c_int, [C.c_int, _vp, _sz, _vp, _vp, _vp]),
    "mbx_synthesize_tone": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_state_copy": (C.c_int, [C.c_int, _vp, _vp]),
    "mbx_process_batch_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_synthesize_speech_host": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "mbx_floattoshort_host": (C.c_int, [_vp, _vp, _sz]),
    "mbx_fec_host": (C.c_int, [C.c_int, _vp, _sz, _vp]),
    "mbx_pack_imbe7100x4400": (C.c_int, [_vp, _sz, _vp]),
    "mbx_fec_imbe7100x4400": (C.c_int, [_vp, _sz, _vp, _vp]),
    "mbx_fec_soft": (C.c_int, [C.c_int, _vp, _sz, _vp, _vp]),
    "mbx_process_batch_soft": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_batch_soft_ws": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mbx_process_batch_soft_resident": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_batch_ragged": (C.c_int, [C.c_int, C.c_int, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_batch_soft_ragged": (C.c_int, [C.c_int, C.c_int, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_batch_mixed": (C.c_int, [C.c_int, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_batch_soft_mixed": (C.c_int, [C.c_int, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_ecc_soft_words": (C.c_int, [C.c_int, _vp, _sz, _vp, _vp, _vp]),
    "mbx_validate_soft_bits": (C.c_int, [_vp, _sz]),
    "mbx_soft_bits_from_hard": (C.c_int, [_vp, _vp, _sz, C.c_uint8]),
    "mbx_soft_bits_from_llr": (C.c_int, [_vp, _vp, _sz]),
    "mbx_fec_soft_host": (C.c_int, [C.c_int, _vp, _sz, _vp]),
    "mbx_process_batch_soft_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_ecc_soft_words_host": (C.c_int, [C.c_int, _vp, _sz, _vp, _vp]),
    "mbx_session_create": (C.c_int, [_vp, C.c_int, C.c_int, _sz, C.c_uint]),
    "mbx_session_destroy": (C.c_int, [_vp]),
    "mbx_session_streams": (C.c_int, [_vp]),
    "mbx_session_submit": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp]),
    "mbx_session_submit_indexed": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_session_submit_soft": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp]),
    "mbx_session_submit_soft_indexed": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_session_wait": (C.c_int, [_vp]),
    "mbx_session_reset": (C.c_int, [_vp, C.c_int, C.c_int]),
    "mbx_session_seed": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "mbx_session_get_state": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_session_set_state": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_host_alloc": (_vp, [_sz]),
    "mbx_host_free": (None, [_vp]),
    "mbx_rng_default": (None, [_vp]),
    "mbx_rng_seed": (None, [_vp, C.c_uint32]),
    "mbx_stream_kernel_name": (C.c_char_p, [C.c_int, C.c_int]),
    "mbx_batch_kernel_name": (C.c_char_p, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mbx_front_fallbacks": (C.c_longlong, [C.c_void_p]),
    "mbx_last_kernel_name": (C.c_char_p, [C.c_void_p]),
    "mbx_launch_slices": (C.c_int, [C.c_int, C.c_int, C.c_int]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
# burst input (include/mbx_burst.h): a table of its own, so that EXPORTED_SYMBOLS stays what include/mbx.h declares
_BURST_SIGNATURES = {
    "mbx_burst_schedule_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    "mbx_burst_schedule_create_form": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp]),
    "mbx_burst_schedule_create_llr": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp]),
    "mbx_burst_schedule_destroy": (C.c_int, [_vp]),
    "mbx_burst_schedule_codec": (C.c_int, [_vp]),
    "mbx_burst_schedule_frames": (C.c_int, [_vp]),
    "mbx_burst_schedule_bits": (C.c_int, [_vp]),
    "mbx_burst_schedule_form": (C.c_int, [_vp]),
    "mbx_burst_schedule_bytes": (_sz, [_vp]),
    "mbx_burst_schedule_soft_cells": (_sz, [_vp]),
    "mbx_burst_schedule_soft_bytes": (_sz, [_vp]),
    "mbx_burst_validate": (C.c_int, [_vp, _vp, _sz, _sz, C.c_int]),
    "mbx_burst_workspace_frames": (_sz, [_vp, C.c_int, C.c_int]),
    "mbx_deinterleave": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _vp]),
    "mbx_deinterleave_soft": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp]),
    "mbx_process_bursts": (C.c_int, [_vp, C.c_int, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_bursts_soft": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_session_submit_bursts": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _sz, _vp, _vp, _vp]),
    "mbx_session_submit_bursts_soft": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
}
BURST_SYMBOLS = tuple(_BURST_SIGNATURES)
# LLR input that is not a burst (include/mbx_llr.h)
_LLR_SIGNATURES = {
    "mbx_soft_from_llr": (C.c_int, [_vp, C.c_int, _sz, _vp, _vp]),
}
LLR_SYMBOLS = tuple(_LLR_SIGNATURES)
# burst groups (include/mbx_burst_groups.h): the bursts of several schedules in one call
_GROUP_SIGNATURES = {
    "mbx_process_burst_groups": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_burst_groups_workspace_frames": (_sz, [_vp, C.c_int, C.c_int]),
    "mbx_burst_groups_rows": (C.c_int, [_vp, C.c_int, _vp]),
    "mbx_session_create_mixed": (C.c_int, [_vp, C.c_int, _vp, _sz, C.c_uint]),
    "mbx_session_submit_burst_groups": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
}
GROUP_SYMBOLS = tuple(_GROUP_SIGNATURES)
# keystream input (include/mbx_keystream.h): encrypted channels on the batched paths
_KEYSTREAM_SIGNATURES = {
    "mbx_keystream_apply_host": (C.c_int, [C.c_int, _vp, _sz, _vp]),
    "mbx_apply_keystream": (C.c_int, [C.c_int, _vp, _sz, _vp, _vp]),
    "mbx_process_batch_keyed": (C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_batch_ragged_keyed": (C.c_int, [C.c_int, _vp, C.c_int, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_session_submit_keyed": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
KEYSTREAM_SYMBOLS = tuple(_KEYSTREAM_SIGNATURES)
# companded PCM out (include/mbx_pcm8.h): G.711 bytes, converted on the device
_PCM8_SIGNATURES = {
    "mbx_pcm_compand_host": (C.c_int, [C.c_int, _vp, _sz, _vp]),
    "mbx_pcm_compand": (C.c_int, [C.c_int, _vp, _sz, _vp, _vp]),
    "mbx_session_next_pcm8": (C.c_int, [_vp, C.c_int, _vp]),
}
PCM8_SYMBOLS = tuple(_PCM8_SIGNATURES)
# mix-down out (include/mbx_mixdown.h): talkgroup buses summed on the device
_MIXDOWN_SIGNATURES = {
    "mbx_mixdown_plan_create": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    "mbx_mixdown_plan_create_split": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.c_int]),
    "mbx_mixdown_plan_destroy": (C.c_int, [_vp]),
    "mbx_mixdown_plan_buses": (C.c_int, [_vp]),
    "mbx_mixdown_plan_rows": (C.c_int, [_vp]),
    "mbx_mixdown_plan_long_buses": (C.c_int, [_vp]),
    "mbx_mixdown_host": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mbx_mixdown": (C.c_int, [_vp, C.c_int, _vp, _sz, _vp, _vp]),
    "mbx_session_next_mixdown": (C.c_int, [_vp, _vp, C.c_int, _vp]),
}
MIXDOWN_SYMBOLS = tuple(_MIXDOWN_SIGNATURES)
# levels out and the gated mix-down (include/mbx_levels.h): a level record per row, buses of the open / the N loudest inputs
_LEVELS_SIGNATURES = {
    "mbx_pcm_levels": (C.c_int, [_vp, _sz, _vp, _vp]),
    "mbx_pcm_levels_host": (C.c_int, [_vp, _sz, _vp]),
    "mbx_mixdown_gated": (C.c_int, [_vp, _vp, C.c_int, _vp, _sz, _vp, _vp, _vp]),
    "mbx_mixdown_gated_host": (C.c_int, [C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mbx_session_next_levels": (C.c_int, [_vp, _vp]),
    "mbx_session_next_mixdown_gated": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
}
LEVELS_SYMBOLS = tuple(_LEVELS_SIGNATURES)
# the held gate (include/mbx_hold.h): the gated mix-down with hysteresis, hang time and ramps, a state record per input on the device
_HOLD_SIGNATURES = {
    "mbx_gate_state_create": (C.c_int, [_vp, _vp]),
    "mbx_gate_state_destroy": (C.c_int, [_vp]),
    "mbx_gate_state_inputs": (C.c_int, [_vp]),
    "mbx_gate_state_reset": (C.c_int, [_vp, _vp]),
    "mbx_gate_state_get": (C.c_int, [_vp, _vp, _vp]),
    "mbx_gate_state_set": (C.c_int, [_vp, _vp, _vp]),
    "mbx_mixdown_held": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _sz, _vp, _vp, _vp]),
    "mbx_mixdown_held_host": (C.c_int, [C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "mbx_session_next_mixdown_held": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp]),
}
HOLD_SYMBOLS = tuple(_HOLD_SIGNATURES)
# levelled rows (include/mbx_agc.h): a per-stream automatic gain over the int16 rows, a state record per stream on the device
_AGC_SIGNATURES = {
    "mbx_agc_state_create": (C.c_int, [_vp, C.c_int]),
    "mbx_agc_state_destroy": (C.c_int, [_vp]),
    "mbx_agc_state_streams": (C.c_int, [_vp]),
    "mbx_agc_state_reset": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "mbx_agc_state_get": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_agc_state_set": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_pcm_agc": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "mbx_pcm_agc_host": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_session_next_agc": (C.c_int, [_vp, _vp, _vp]),
}
AGC_SYMBOLS = tuple(_AGC_SIGNATURES)
# limited buses (include/mbx_limit.h): the int32 sums of the bus launches and a look-ahead peak limiter behind them, a state record per bus
_LIMIT_SIGNATURES = {
    "mbx_limit_state_create": (C.c_int, [_vp, C.c_int]),
    "mbx_limit_state_destroy": (C.c_int, [_vp]),
    "mbx_limit_state_buses": (C.c_int, [_vp]),
    "mbx_limit_state_reset": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "mbx_limit_state_get": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_limit_state_set": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_limit_state_sums": (_vp, [_vp]),
    "mbx_bus_limit": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp]),
    "mbx_bus_limit_host": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp]),
    "mbx_mixdown_sums": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "mbx_mixdown_sums_host": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mbx_mixdown_gated_sums": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "mbx_mixdown_gated_sums_host": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mbx_mixdown_held_sums": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "mbx_mixdown_held_sums_host": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "mbx_session_next_limit": (C.c_int, [_vp, _vp, _vp]),
}
LIMIT_SYMBOLS = tuple(_LIMIT_SIGNATURES)
# wide rows (include/mbx_resample.h): int16 rows upsampled by a polyphase FIR interpolator, a 64-byte history record per row on the device
_RESAMPLE_SIGNATURES = {
    "mbx_resample_state_create": (C.c_int, [_vp, C.c_int]),
    "mbx_resample_state_destroy": (C.c_int, [_vp]),
    "mbx_resample_state_streams": (C.c_int, [_vp]),
    "mbx_resample_state_reset": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "mbx_resample_state_get": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_resample_state_set": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_pcm_resample": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "mbx_pcm_resample_host": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_session_next_resample": (C.c_int, [_vp, _vp, _vp, _vp]),
}
RESAMPLE_SYMBOLS = tuple(_RESAMPLE_SIGNATURES)
# filtered rows (include/mbx_filter.h): a per-stream biquad cascade over the int16 rows, a 32-byte state record per stream on the device
_FILTER_SIGNATURES = {
    "mbx_filter_state_create": (C.c_int, [_vp, C.c_int]),
    "mbx_filter_state_destroy": (C.c_int, [_vp]),
    "mbx_filter_state_streams": (C.c_int, [_vp]),
    "mbx_filter_state_reset": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "mbx_filter_state_get": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_filter_state_set": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_pcm_filter": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "mbx_pcm_filter_host": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]),
    "mbx_session_next_filter": (C.c_int, [_vp, _vp, _vp]),
}
FILTER_SYMBOLS = tuple(_FILTER_SIGNATURES)
# band records (include/mbx_bands.h): the int16 rows against a caller's bank of probes, K small records per row; the bank on the device
_BANDS_SIGNATURES = {
    "mbx_band_bank_create": (C.c_int, [_vp, _vp, C.c_int]),
    "mbx_band_bank_destroy": (C.c_int, [_vp]),
    "mbx_band_bank_probes": (C.c_int, [_vp]),
    "mbx_pcm_bands": (C.c_int, [_vp, C.c_int, _vp, _sz, _vp, _vp]),
    "mbx_pcm_bands_host": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _sz, _vp]),
    "mbx_session_next_bands": (C.c_int, [_vp, _vp, C.c_int, _vp]),
}
BANDS_SYMBOLS = tuple(_BANDS_SIGNATURES)
# voted streams (include/mbx_vote.h): several receivers' copies of a frame picked on their records or combined on their cells; the grouping on the device
_VOTE_SIGNATURES = {
    "mbx_vote_plan_create": (C.c_int, [_vp, _vp, C.c_int]),
    "mbx_vote_plan_destroy": (C.c_int, [_vp]),
    "mbx_vote_plan_streams": (C.c_int, [_vp]),
    "mbx_vote_plan_candidates": (C.c_int, [_vp]),
    "mbx_vote_select": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "mbx_vote_combine": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "mbx_vote_select_host": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "mbx_vote_combine_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "mbx_vote_workspace_frames": (_sz, [_vp, C.c_int, C.c_int, C.c_int]),
    "mbx_process_batch_voted": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mbx_process_batch_soft_voted": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
VOTE_SYMBOLS = tuple(_VOTE_SIGNATURES)


class BurstGroupStruct(C.Structure):
    """mbx_burst_group"""
    _fields_ = [("sched", _vp), ("bursts", _vp), ("burst_stride", _sz), ("n_streams", C.c_int), ("bursts_per_stream", C.c_int),
                ("stream_index", _vp), ("first_slot", C.c_int)]


def lib():
    """The loaded library handle (loads on first use)."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise NativeLibraryError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  mbelib-neo_amd has no CPU fallback."
            )
        # torch ships its own HIP runtime; load it first so that this library binds to the SAME
        # libamdhip64 instance (device pointers and streams are shared with torch tensors).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        try:
            handle = C.CDLL(path)
        except OSError as e:  # e.g. libamdhip64 not found
            raise NativeLibraryError(f"cannot load {path}: {e}") from e
        for name, (res, args) in {**_SIGNATURES, **_BURST_SIGNATURES, **_LLR_SIGNATURES, **_GROUP_SIGNATURES, **_KEYSTREAM_SIGNATURES, **_PCM8_SIGNATURES,
                                   **_MIXDOWN_SIGNATURES, **_LEVELS_SIGNATURES, **_HOLD_SIGNATURES, **_AGC_SIGNATURES, **_LIMIT_SIGNATURES,
                                   **_RESAMPLE_SIGNATURES, **_FILTER_SIGNATURES, **_BANDS_SIGNATURES, **_VOTE_SIGNATURES}.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                if os.environ.get("MBX_HIP_LIBRARY_ALLOW_OLDER") == "1":   # tools/abx.sh: A/B against a library of an earlier commit
                    continue
                raise NativeLibraryError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        if hasattr(handle, "mbx_testing_set_front_skip"):   # libmbx_hip_testing.so only (tests/front_skip_case.py)
            handle.mbx_testing_set_front_skip.restype = C.c_int
            handle.mbx_testing_set_front_skip.argtypes = [C.c_int]
        if hasattr(handle, "mbx_debug_set_ablation"):   # development build only
            handle.mbx_debug_set_ablation.restype = None
            handle.mbx_debug_set_ablation.argtypes = [C.c_int]
        _lib = handle
    return _lib


def check(rc, what):
    if rc < 0:
        msg = lib().mbx_last_error()
        raise NativeLibraryError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")
    return rc
