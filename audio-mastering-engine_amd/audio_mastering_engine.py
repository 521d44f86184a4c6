"""Drop-in replacement module for the reference's mastering entry points.

Mirrors audio_mastering_engine.py's call surface for the hot path:

* ``master_audio(settings, status_callback=None, progress_callback=None) -> str``
  -- the semantics of ``process_audio_with_ffmpeg_pipeline`` (:171-226): same
  ``settings`` keys and defaults, same status strings and progress sequence
  (``(0,100)``, ``(i+1, n+4)`` per chunk, ``n+1``, ``n+2`` only with ``lufs``,
  ``n+3``, ``n+4``), same ``ValueError`` for missing files, writes a 16-bit WAV -- or,
  for an ``output_file`` named ``*.flac``, a 16-bit FLAC file encoded on the device
  (optional key ``flac_lpc_order`` 0..8: LPC subframes up to that order; absent: 0).
  The optional key ``flac_decode`` says where a ``*.flac`` input is decoded: ``"host"``
  (absent: the host decoder and an upload of the decoded samples) or ``"device"`` (the
  file's bytes go up and are decoded there); any other value is a ``ValueError``.
  The optional key ``multichannel_dynamic`` (a bool, absent: ``False``) lets a file with 3
  to 8 channels take loudnorm's dynamic mode (a 192 kHz master, like a stereo file's)
  where it otherwise ends in ``DynamicModeUnsupported``; any other value is a ``ValueError``.
* ``process_audio_with_ffmpeg_pipeline`` -- alias of ``master_audio``.
* ``process_audio(settings, status_cb, progress_cb, art_cb, tag_cb)`` -- the GUI
  wrapper (:94-137): mastering, the optional MP3 export (:97-98, ``export_to_mp3``
  :140-150, through an ``ffmpeg`` on PATH exactly as the reference calls it), and
  the AI/art branches out of scope: it reports
  ``"Success: Processing complete! (No art generated)"``, ``art_callback(None)``;
  on any error ``"Error: ..."``, ``progress(0, 1)``, ``art(None)``,
  ``tag("Processing failed.")`` exactly like :131-137.
* ``EQ_PRESETS`` (:32-38).
* ``master_files(jobs, ...)`` -- a list of ``master_audio`` settings dicts in one call: the
  files are read ahead and written behind on threads and those that can share a plan run
  as one batch (amx/files.py); every output file is ``master_audio``'s.

All per-sample work runs on the GPU (libamx.so via amx.engine): the host parses the
WAV container and moves the file's own bytes to the device; the s16 conversion of
ffmpeg's split (any PCM format, mono duplicated) is a kernel (amx_pcm_to_s16), and a
float32 file goes straight into the chain, whose first kernel quantises it.
"""
import logging
import os
import subprocess
import sys
import traceback

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import numpy as np  # noqa: E402

from amx import wavio  # noqa: E402
from amx.chunking import bounds_for  # noqa: E402
from amx.settings import EQ_PRESETS, flac_decode_mode, multichannel_dynamic, output_rate  # noqa: E402,F401

__all__ = ["master_audio", "process_audio", "process_audio_with_ffmpeg_pipeline", "EQ_PRESETS",
           "master_array", "export_to_mp3", "master_files"]


def _noop(*a, **k):
    return None


def _flac_on_device(path):
    """read_audio_raw's FLAC result with the samples decoded on, and left on, the device:
    (int32 device tensor [frames, channels], WavInfo of s32 PCM with packet_starts, "s32")"""
    from amx import flacio
    with open(path, "rb") as f:
        x, finfo, blocks = flacio.decode_flac_device(f.read())
    info = wavio.WavInfo(finfo.sample_rate, finfo.channels, 1, 32)
    info.packet_starts = np.concatenate([[0], np.cumsum(blocks.astype(np.int64))[:-1]])
    return x, info, "s32"


def _device_input(path, settings=None, on_info=None):
    """The input file on the device, as the chunk chain reads it: (d_in, fs, frames,
    channels_in, input_s16, WavInfo).  on_info(sample_rate, channels) is called once the
    header is known, before the samples go to the device or a conversion kernel runs (a
    FLAC file decoded on the device: after its decode).  float32 stays float32 (the chain's
    first kernel quantises it, A.1); every other format is decoded to stereo s16 by
    amx_pcm_to_s16 (what ffmpeg's split writes + pydub's set_channels(2)).  With the
    settings key flac_decode = "device" a FLAC file's samples never exist on the host:
    amx_pcm_to_s16 reads the device decoder's array."""
    import torch
    from amx import flacio
    if flac_decode_mode(settings) == "device" and flacio.is_flac(path):
        d_raw, info, code = _flac_on_device(path)
        frames = int(d_raw.shape[0])
    else:
        raw, info, code = wavio.read_audio_raw(path)      # WAV, AIFF / AIFF-C or FLAC
        frames = raw.size // info.block_align
        d_raw = None
    if not 1 <= info.channels <= 8:
        raise ValueError("1 to 8 channels are supported (%d channels)" % info.channels)
    if on_info is not None:
        on_info(info.sample_rate, info.channels)
    if d_raw is None:
        d_raw = torch.from_numpy(raw.copy()).to("cuda")
    d_in, ch_in, s16 = _chain_input(d_raw, info.channels, code, frames)
    return d_in, info.sample_rate, frames, ch_in, s16, info


def _chain_input(d_raw, channels, code, frames, out=None):
    """The file's samples on the device (d_raw: its bytes, or the device FLAC decoder's
    array) as the chain input: (d_in, channels_in, input_s16).  out: an int16 device tensor
    [frames, channels_in] that amx_pcm_to_s16 writes into when it runs (None: a new one)."""
    import torch
    from amx import capi
    ch_in, s16, direct = wavio.chain_kind(channels, code)
    if direct:
        return d_raw.view(torch.int16 if s16 else torch.float32), ch_in, s16
    d_in = out if out is not None else torch.empty((max(1, frames), ch_in), dtype=torch.int16, device="cuda")
    capi.check(capi.load().amx_pcm_to_s16(capi.ptr(d_raw), frames, channels,
                                          capi.PCM_FORMATS[code], capi.ptr(d_in),
                                          capi.ptr_stream()), "amx_pcm_to_s16")
    return d_in, ch_in, s16


def _write_output(path, y_device, fs, settings=None):
    """The mastered int16 track (a device tensor) as the file ffmpeg's last command writes
    (:223, `-y output_file`: the extension picks the container): *.flac in any letter case
    is encoded on the device (amx.flacio.write_flac, with STREAMINFO's MD5); every other
    name gets the 16-bit WAV.  The optional settings key flac_lpc_order (0..8, absent: 0,
    the FIXED-only file) is write_flac's lpc_order; a name that is not *.flac ignores it."""
    if os.path.splitext(str(path))[1].lower() == ".flac":
        from amx import flacio
        flacio.write_flac(path, y_device, fs, lpc_order=(settings or {}).get("flac_lpc_order", 0))
    else:
        wavio.write_wav_s16(path, y_device.cpu().numpy(), fs)


def _normalize(job):
    """normalize_loudness_on_disk_with_ffmpeg (:227-242) on the device: the rest of pass
    1's measurement, the statistics and decision; dynamic mode (:240 when the linear
    conditions fail) runs the 192 kHz path and returns its (output, info), linear
    mode (and the -inf skip, :238) returns None -- the gain rides in amx_finalize."""
    job.loudness_pass2(carry=False)
    job.histograms()
    job.decide()
    report = job.fetch_report(raise_dynamic=False)
    mode = report["modes"][0] if report["modes"] else "off"
    if mode == "skip":
        logging.warning("Measured loudness is -inf (silent audio). Skipping normalization.")
    if mode == "dynamic":
        # loudnorm pass 2 in dynamic mode (:240): 192 kHz AGC + true-peak limiter
        return job.dynamic_track(0, report["stats"][0])
    return None


def _normalize_multichannel(job):
    """_normalize for a MultiChannelJob (settings key multichannel_dynamic): the
    measurement and decision; dynamic mode returns MultiChannelJob.dynamic's (output, info),
    linear mode and the -inf skip None"""
    job.measure(lufs_on=True)
    report = job.fetch_report(raise_dynamic=False)
    mode = report["modes"][0] if report["modes"] else "off"
    if mode == "skip":
        logging.warning("Measured loudness is -inf (silent audio). Skipping normalization.")
    if mode == "dynamic":
        return job.dynamic(report["stats"][0])
    return None


def _check_settings(settings):
    """what master_audio refuses before any file is read"""
    if not settings.get("input_file") or not settings.get("output_file"):
        raise ValueError("Input or output file not specified.")              # :173
    flac_decode_mode(settings)                         # a bad flac_decode: before any file is read
    output_rate(settings, 0)                           # a bad output_rate likewise
    multichannel_dynamic(settings)                     # and a bad multichannel_dynamic


def master_audio(settings, status_callback=None, progress_callback=None):
    from amx.engine import delivery_rate

    status = status_callback or _noop
    progress = progress_callback or _noop
    _check_settings(settings)
    input_file, output_file = settings["input_file"], settings["output_file"]
    # a master rate the resampler cannot take to output_rate: before any kernel runs
    check = lambda rate, channels: delivery_rate(settings, rate, channels)   # noqa: E731
    status("Splitting audio into manageable chunks...")                       # :176
    progress(0, 100)                                                          # :177
    d_in, fs, frames, ch_in, s16, info = _device_input(input_file, settings, check)
    target = output_rate(settings, fs)
    bounds = bounds_for(frames, fs, info)                                     # :178
    status("Splitting complete.")                                             # :180
    return _master_device(settings, status, progress, d_in, fs, frames, ch_in, s16, bounds, output_file, target)


def _master_device(settings, status, progress, d_in, fs, frames, ch_in, s16, bounds, output_file, target,
                   write=None, result=None):
    """master_audio from "Splitting complete." on: the input is on the device (d_in, as
    _device_input returns it) and split at `bounds`.  write(path, y_device, fs, settings):
    what takes the finished master (None: _write_output); result: a dict that receives
    mode, stats (the pass-1 strings or None) and sample_rate (as delivered) -- master_files
    (amx.files) runs a file that is alone in its group through this very sequence."""
    import torch
    from amx.engine import MasteringJob, deliver
    write = write or _write_output
    num_chunks = len(bounds)
    total_steps = num_chunks + 4                                              # :184
    if ch_in > 2:
        return _master_multichannel(settings, status, progress, d_in, fs, frames, ch_in, s16, bounds,
                                    output_file, target, write, result)
    job = MasteringJob(fs, ch_in, settings, [frames], input_s16=s16,
                       chunks=[(0, s, n) for s, n in bounds])
    # every chunk's chain runs in the same launches (chunks are independent,
    # :185-204); the per-chunk callbacks fire while the device works on them and
    # "Re-assembling" fires once the chain is done
    if num_chunks:
        job.run_chunks(d_in)
    for i in range(num_chunks):
        status(f"Processing chunk {i+1} of {num_chunks}...")                  # :186
        progress(i + 1, total_steps)                                          # :187
    torch.cuda.current_stream().synchronize()
    status("Re-assembling processed chunks with concat filter...")           # :205
    progress(num_chunks + 1, total_steps)                                     # :206
    status("Concatenation complete.")                                         # :213
    # the sample peaks the limiter's path decision needs (and, with lufs, the first
    # half of loudnorm's 192 kHz measurement)
    job.loudness_pass1()
    dyn = None
    report = {}
    if settings.get("lufs") is not None:                                      # :216
        status("Normalizing final loudness...")                               # :217
        progress(num_chunks + 2, total_steps)                                 # :218
        try:
            dyn = _normalize(job)
            report = job.report
        except Exception as e:                                                # :243-246
            # the reference logs any normalisation error and carries on with a copy of
            # the unnormalised track: here the track is finalised without the gain
            logging.exception("Error during disk-based normalization.")
            if isinstance(e, subprocess.CalledProcessError):
                logging.error(f"FFMPEG STDERR:\n{e.stderr}")
            dyn = None
            job.dd.lufs_on = 0
            job.decide()
    else:
        job.decide()
    status("Applying final limiting and exporting...")                        # :221
    progress(num_chunks + 3, total_steps)                                     # :222
    if dyn is None:
        job.finalize(None)
        y, out_fs = job.y[:job.info.out_frames], fs
    else:
        # the alimiter ran on the 192 kHz file inside dynamic_track (:223 keeps its rate)
        y, out_fs = dyn[0], dyn[1]["sample_rate"]
    rate = {"sample_rate": out_fs}
    y = deliver(y, rate, target)                       # output_rate: the resampler after the alimiter
    _fill_result(result, report, rate)
    write(output_file, y, rate["sample_rate"], settings)
    progress(total_steps, total_steps)                                        # :224
    logging.info(f"Finished GPU pipeline, exported to {output_file}")
    return output_file


def _fill_result(result, report, rate):
    """_master_device's `result`: the loudness decision of the one track (report:
    fetch_report's, empty when the stage did not run or failed) and the delivered rate"""
    if result is not None:
        modes, stats = report.get("modes"), report.get("stats")
        result.update(mode=modes[0] if modes else "off", stats=stats[0] if stats else None,
                      sample_rate=int(rate["sample_rate"]))


def _master_multichannel(settings, status, progress, d_in, fs, frames, channels, s16, bounds, output_file,
                         target=None, write=None, result=None):
    """master_audio for a file with 3..8 channels: the chain over the interleaved stream
    (:252), the measurement over the C channels and the C-channel alimiter
    (amx.engine.MultiChannelJob), with the same status strings and progress sequence.
    Loudnorm's dynamic mode raises DynamicModeUnsupported for such a file unless the
    settings key multichannel_dynamic is True: then MultiChannelJob.dynamic runs it (the
    master is at 192 kHz), and -- as for stereo, :243-246 -- an error in the loudness stage
    is logged and the track finalised without the gain.  target: the delivery rate
    (settings key output_rate), None: the master's own.  write, result: as in _master_device."""
    import torch
    from amx.engine import MultiChannelJob, deliver
    write = write or _write_output
    num_chunks = len(bounds)
    total_steps = num_chunks + 4
    job = MultiChannelJob(fs, channels, settings, frames, input_s16=s16, chunks=[(0, s, n) for s, n in bounds])
    if num_chunks:
        job.run_chunks(d_in)
    for i in range(num_chunks):
        status(f"Processing chunk {i+1} of {num_chunks}...")                  # :186
        progress(i + 1, total_steps)                                          # :187
    torch.cuda.current_stream().synchronize()
    status("Re-assembling processed chunks with concat filter...")           # :205
    progress(num_chunks + 1, total_steps)                                     # :206
    status("Concatenation complete.")                                         # :213
    dyn = None
    report = {}
    if settings.get("lufs") is not None:                                      # :216
        status("Normalizing final loudness...")                               # :217
        progress(num_chunks + 2, total_steps)                                 # :218
        if multichannel_dynamic(settings):
            try:
                dyn = _normalize_multichannel(job)
                report = job.report
            except Exception as e:                                            # :243-246
                logging.exception("Error during disk-based normalization.")
                if isinstance(e, subprocess.CalledProcessError):
                    logging.error(f"FFMPEG STDERR:\n{e.stderr}")
                dyn = None
                job.measure(lufs_on=False)
        else:
            job.measure(lufs_on=True)
            rep = report = job.fetch_report(raise_dynamic=True)
            if rep["modes"] and rep["modes"][0] == "skip":
                logging.warning("Measured loudness is -inf (silent audio). Skipping normalization.")
    else:
        job.measure(lufs_on=False)
    status("Applying final limiting and exporting...")                        # :221
    progress(num_chunks + 3, total_steps)                                     # :222
    if dyn is None:
        rate = {"sample_rate": fs}
        y = job.finalize()
    else:
        # the alimiter ran on the 192 kHz file inside dynamic() (:223 keeps its rate)
        rate = {"sample_rate": dyn[1]["sample_rate"]}
        y = dyn[0]
    y = deliver(y, rate, target)
    _fill_result(result, report, rate)
    write(output_file, y, rate["sample_rate"], settings)
    progress(total_steps, total_steps)                                        # :224
    logging.info(f"Finished GPU pipeline, exported to {output_file}")
    job.close()
    return output_file


process_audio_with_ffmpeg_pipeline = master_audio


def export_to_mp3(input_wav_path, status_callback):
    """:140-150 as the reference does it: the external ffmpeg encodes the mastered
    WAV to VBR MP3 (-q:a 0); a missing ffmpeg fails the same way (status
    "Error: Failed to create MP3 file.")."""
    if not input_wav_path or not os.path.exists(input_wav_path):
        logging.warning("Input WAV file not found for MP3 conversion.")
        status_callback("Warning: Could not find master WAV to create MP3.")
        return
    output_mp3_path = os.path.splitext(input_wav_path)[0] + ".mp3"
    status_callback("Creating high-quality MP3...")
    logging.info(f"Exporting WAV to MP3: {input_wav_path} -> {output_mp3_path}")
    try:
        mp3_command = ['ffmpeg', '-i', input_wav_path, '-q:a', '0', '-y', output_mp3_path]
        subprocess.run(mp3_command, check=True, capture_output=True, text=True)
        logging.info("MP3 export successful.")
        status_callback("High-quality MP3 created successfully.")
    except Exception:
        logging.exception("Error during MP3 export.")
        status_callback("Error: Failed to create MP3 file.")


def process_audio(settings, status_callback, progress_callback, art_callback, tag_callback):
    """:94-137 with the AI / art branches out of scope."""
    try:
        output_wav_path = master_audio(settings, status_callback, progress_callback)
        if settings.get("create_mp3", False):                                 # :97-98
            export_to_mp3(output_wav_path, status_callback)
        status_callback("Mastering complete. Preparing for AI analysis...")
        status_callback("Success: Processing complete! (No art generated)")
        art_callback(None)
    except Exception as e:
        logging.error(f"FATAL ERROR in process_audio: {traceback.format_exc()}")
        status_callback(f"Error: {e}")
        progress_callback(0, 1)
        art_callback(None)
        tag_callback("Processing failed.")


def master_array(x, sample_rate, settings, **kw):
    from amx.engine import master_array as _m
    return _m(x, sample_rate, settings, **kw)


def master_files(jobs, status_callback=None, progress_callback=None, *, workers=None, staging_bytes=None,
                 max_group_frames=None):
    """master_audio for a list of settings dicts, with the host I/O overlapped and the
    files that can share a plan batched (amx/files.py).  Every output file
    is byte for byte the file master_audio(job) writes.

    status_callback(index, message) and progress_callback(index, current, total): per job
    index master_audio's own sequence; the sequences of different files may interleave, and
    both are only ever called from the calling thread.

    Returns one dict per job, in job order: index, input_file, output_file, error (None, or
    the exception master_audio would have raised for that dict -- the other jobs still
    finish, and a failed job leaves no output file), sample_rate (as delivered), mode
    ("linear", "dynamic", "skip", "off"), stats (the pass-1 strings or None) and group (an
    int: jobs that ran in one batched plan share it).  Only a `jobs` that is not a list of
    dicts (TypeError), two jobs naming one output_file (ValueError) and a bad keyword
    argument raise from the call itself, before any file is read.

    workers: the I/O threads (default min(8, jobs), at most 16); staging_bytes: the bound on
    pinned staging memory, half for reading ahead and half for writing behind (default
    2 GiB; a larger file is staged alone); max_group_frames: the most frames in one plan
    (default: what fits in half of the free device memory)."""
    from amx import files
    return files.master_files(sys.modules[__name__], jobs, status_callback, progress_callback, workers=workers,
                              staging_bytes=staging_bytes, max_group_frames=max_group_frames)
