// HipLiveControl.java -- the native methods behind FUNcubeBPSKDemod.actionPerformed (FUNcubeBPSKDemod.java:165-190) and
// setup() (:192-209) on a live handle of HipNative.bpskCreate (jni/jsdr_jni.c -> jsdr_bpsk_set_tuning / _set_mode /
// _reconfigure, include/jsdr_hip.h).  A class of its own beside HipNative: HipNative's set of natives is the fixed surface
// of the four plugin classes and the group (its count is checked, tests/test_jni_sources.py); these three belong to the
// live-control actions only.  Both classes load the same libjsdr_jni.so (a second System.loadLibrary of it is a no-op).
// The change takes effect from the next sample of the next receive(); no other state is reset.  A failed call throws
// IllegalStateException with the library's message and leaves the handle as it was.
package com.ashbysoft.java_sdr;

final class HipLiveControl {
    static {
        System.loadLibrary("jsdr_jni");
    }

    private HipLiveControl() {
    }

    /** tuning = tuningHz; tuPhaseInc = 2 pi tuning / rate; dmMaxCorr = 0 (:177-181,188-190) */
    static native void bpskSetTuning(long h, double tuningHz);
    /** doFFT / doUp as given; tuPhaseInc recomputed; dmMaxCorr = 0 (:182-190) */
    static native void bpskSetMode(long h, int doFFT, int doUp);
    /** setup() on an unchanged AudioDescriptor: the configuration's tuning / doFFT / doUp, dmMaxCorr kept (:192-209) */
    static native void bpskReconfigure(long h, double tuningHz, int doFFT, int doUp);
}
