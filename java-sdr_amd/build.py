#!/usr/bin/env python3
"""Build libjsdr_hip.so (gfx950 only) in-tree with hipcc.  No CPU fallback is built.

    python java-sdr_amd/build.py [--force] [--verbose]

Per-file flags: the exact-order FP64 translation units are compiled with -ffp-contract=off so that
every multiply and add rounds separately, as Java's do.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
OUT = os.path.join(HERE, "libjsdr_hip.so")

COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
          "-Wno-unused-result"]
SOURCES = {
    # (the units that compile longest first: the four workers start in this order, and the last one to finish is the build's wall time.
    #  The tune-mode pipeline is cut by kernel family -- bpsk_front_reg / bpsk_fm / bpsk_fm_f32 / bpsk_front / bpsk_tail -- so that none of them is the
    #  whole build)
    "bpsk_front_reg.hip": ["-ffp-contract=off"],
    # (no atomic optimiser, as for bpsk_acq.hip below: k_fm's and k_fm_f32's ticket is wanted a front half after it is asked for)
    "bpsk_fm.hip": ["-ffp-contract=off", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None"],
    "bpsk_fm_f32.hip": ["-ffp-contract=off", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None"],
    "bpsk_front.hip": ["-ffp-contract=off"],
    "bpsk_tail.hip": ["-ffp-contract=off"],
    "runtime.hip": [],
    "fft_psd.hip": [],
    "fft_mixed.hip": [],
    "fft_any.hip": ["-ffp-contract=off"],
    "fft_rt.hip": [],
    "fir_phase.hip": ["-ffp-contract=off"],
    # (the batched phase scope: the schedule's float recurrence, the column sums, quotients and products round one by one)
    "phase_scope.hip": ["-ffp-contract=off"],
    "fir_batch.hip": ["-ffp-contract=off"],
    "fec.hip": [],
    "synth.hip": [],
    "formats.hip": [],
    "demod.hip": ["-ffp-contract=off"],
    "demod_chan.hip": ["-ffp-contract=off"],
    # (the demod scope: demod.hip's tile again, the column schedules' float products and the painters' casts)
    "demod_scope.hip": ["-ffp-contract=off"],
    # (the handle's units, bpsk_handle.h: host code only, but tuPhaseInc and its sin / cos tables are doubles that must round as Java's do)
    "bpsk_call.hip": ["-ffp-contract=off"],
    "bpsk_handle.hip": ["-ffp-contract=off"],
    "bpsk_control.hip": ["-ffp-contract=off"],
    "bpsk_results.hip": ["-ffp-contract=off"],
    "bpsk_call_chan.hip": ["-ffp-contract=off"],
    "bpsk_ckpt.hip": ["-ffp-contract=off"],
    "bpsk_call_pst.hip": ["-ffp-contract=off"],
    # (the host scheduler: host code only, it steps the reference's phase recurrences in doubles that must round as Java's do)
    "bpsk_sched.hip": ["-ffp-contract=off"],
    # (the demod handle's units, demod_handle.h: host code only; the weights and the carrier phases are floats that must round as Java's do)
    # (demod_call.hip holds the carrier walk, a 7-instruction loop that has to retire one float subtraction's latency an iteration:
    #  kept inside one 32-byte fetch block wherever the unit lands in the library)
    "demod_call.hip": ["-ffp-contract=off", "-falign-loops=32"],
    "demod_control.hip": ["-ffp-contract=off"],
    "demod_scope_host.hip": ["-ffp-contract=off"],
    "demod_host.hip": ["-ffp-contract=off"],
    "bpsk_fft.hip": ["-ffp-contract=off"],
    # (no atomic optimiser: it turns the one-lane ticket atomicAdd into atomic + s_waitcnt vmcnt(0) + v_readfirstlane on the spot,
    #  i.e. a round trip to memory at the top of a frame for a value that is wanted a pass later)
    "bpsk_acq.hip": ["-ffp-contract=off", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None"],
    "bpsk_acq_chan.hip": ["-ffp-contract=off", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None"],
    # (the mixed-radix front ends, cut by kernel family over bpsk_fftm_dev.h's passes)
    "bpsk_fftm.hip": ["-ffp-contract=off"],
    "bpsk_fft2x.hip": ["-ffp-contract=off"],
    "bpsk_fftm2.hip": ["-ffp-contract=off"],
    "bpsk_acqg.hip": ["-ffp-contract=off"],
    # (the FFT-acquire plan: host code only; its twiddle tables are long doubles rounded once -- flagged like its neighbours)
    "bpsk_fftplan.hip": ["-ffp-contract=off"],
    "bpsk_chan.hip": ["-ffp-contract=off"],
    "bpsk_pst.hip": ["-ffp-contract=off"],
    "bpsk_chan_pst.hip": ["-ffp-contract=off"],
    # (checkpoints: the gather / scatter kernels do no arithmetic; the blob codec is host code only -- flagged like their neighbours)
    "bpsk_state.hip": ["-ffp-contract=off"],
    "bpsk_blob.hip": ["-ffp-contract=off"],
    # (the BPSK scope: the painter's rings and integers, every product, sum and quotient one IEEE double operation; its host side with it)
    "bpsk_scope.hip": ["-ffp-contract=off"],
    # (the scope's two spectra: the oracle's FP64 transform of a row in LDS, operation for operation, magnitudes and casts behind it)
    "bpsk_scope_spec.hip": ["-ffp-contract=off"],
    "group.hip": [],
}


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "jsdr_hip.h"))
    headers.append(os.path.abspath(__file__))
    jobs = []
    objs = []
    for src, extra in SOURCES.items():
        sp = os.path.join(CSRC, src)
        if not os.path.exists(sp):
            continue
        op = os.path.join(OBJ, src.replace(".hip", ".o"))
        objs.append(op)
        if force or newer(op, [sp] + headers):
            jobs.append([hipcc()] + COMMON + extra + ["-c", sp, "-o", op])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        return r.stderr

    with ThreadPoolExecutor(max_workers=4) as ex:
        for warn in ex.map(run, jobs):
            if verbose and warn.strip():
                print(warn)
    if force or jobs or newer(OUT, objs):
        run([hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs + ["-Wl,-rpath,/opt/rocm/lib", "-ldl", "-lpthread"])
    return OUT


if __name__ == "__main__":
    p = build(force="--force" in sys.argv, verbose="--verbose" in sys.argv)
    print(p)
