// HipFUNcubeBPSKDemod.java -- FUNcubeBPSKDemod's receive chain (FUNcubeBPSKDemod.java:357-595) and FECDecoder on the
// MI355X.  Constructor as jsdr.java:479-483 builds the reference class; the same three configuration keys
// (:102-104,195-200); the same publications (:377-378,455-456); the painted fields (:220-228,331-337) through getters.
// It is a tab like the class it replaces (jsdr.java:479-483: tabs.add(nm, new FUNcubeBPSKDemod(...)) takes a Swing
// component): it extends IUIComponent as FUNcubeBPSKDemod.java:24 does, with hotKey and a paintComponent that draws the
// text statistics of :220-228 and the decoded frame of :331-337 from the lock-free snapshot.
package com.ashbysoft.java_sdr;

import java.awt.Color;
import java.awt.Graphics;

public class HipFUNcubeBPSKDemod extends IUIComponent implements IAudioHandler, IRawHandler, IPublishListener {
    private static final String CFG_TUNING = "bpsk-tuning";
    private static final String CFG_DOFFT = "bpsk-dofft";
    private static final String CFG_UPPER = "bpsk-upper";

    private final String name;
    private final IConfig config;
    private final IPublish publish;
    private final ILogger logger;
    private final boolean rawPath;
    private IAudio audio;
    private long handle;
    private AudioDescriptor audioDesc;
    private double tuning;   // a double, as the reference's: "bpsk-freq" may give what +-10 never reaches
    private boolean doFFT, doUp;
    // results of the last completed receive(), refreshed through HipNative.bpskSnapshot -- a lock-free host-side read
    // (no device call), so the painting thread never waits for the GPU and never blocks the audio thread
    private final Object resultLock = new Object();
    private final int[] counters = new int[11];   // ten counters + the number of bits sliced in that frame
    private final byte[] decoded = new byte[256];
    private final double[] state = new double[18];
    private final byte[] bits = new byte[512];

    public HipFUNcubeBPSKDemod(int idx, IConfig cfg, IPublish pub, ILogger log, IUIHost hst, IAudio aud) {
        this(idx, cfg, pub, log, hst, aud, false);
    }

    public HipFUNcubeBPSKDemod(int idx, IConfig cfg, IPublish pub, ILogger log, IUIHost hst, IAudio aud, boolean rawPath) {
        this.name = "FUNcube" + idx;
        this.config = cfg;
        this.publish = pub;
        this.logger = log;
        this.rawPath = rawPath;
        setup(aud);
        pub.listen(this);
    }

    public void notify(String key, Object val) {
        if ("audio-change".equals(key) && val instanceof IAudio)
            setup((IAudio) val);
    }

    /** the menu actions of :177-190 on the live handle: the tuner, the band and the front end change from the next sample on,
     *  every other piece of state (the down-sampler, matched filter and bit clock, the FEC register, the counters) carries on */
    public synchronized void plus10() {
        setFrequency(tuning + 10.0);
    }

    public synchronized void sub10() {
        setFrequency(tuning - 10.0);
    }

    /** "bpsk-freq": what freqDialog returned */
    public synchronized void setFrequency(double hz) {
        HipLiveControl.bpskSetTuning(handle, hz);
        tuning = hz;
        config.setIntConfig(name + "-" + CFG_TUNING, (int) tuning);
    }

    /** "bpsk-fft-tune": the same handle switches front ends, its down-sampler history carried across exactly */
    public synchronized void toggleFft() {
        HipLiveControl.bpskSetMode(handle, doFFT ? 0 : 1, doUp ? 1 : 0);
        doFFT = !doFFT;
        config.setIntConfig(name + "-" + CFG_DOFFT, doFFT ? 1 : 0);
        config.setIntConfig(name + "-" + CFG_TUNING, (int) tuning);
    }

    /** "bpsk-high" */
    public synchronized void toggleHigh() {
        HipLiveControl.bpskSetMode(handle, doFFT ? 1 : 0, doUp ? 0 : 1);
        doUp = !doUp;
        config.setIntConfig(name + "-" + CFG_UPPER, doUp ? 1 : 0);
        config.setIntConfig(name + "-" + CFG_TUNING, (int) tuning);
    }

    private synchronized void setup(IAudio aud) {
        AudioDescriptor ad = aud.getAudioDescriptor();
        int newTuning = config.getIntConfig(name + "-" + CFG_TUNING, 12000);
        boolean newFFT = 0 != config.getIntConfig(name + "-" + CFG_DOFFT, 0);
        boolean newUp = 0 != config.getIntConfig(name + "-" + CFG_UPPER, 0);
        if (handle != 0 && audio != null && sameFormat(ad, audioDesc)) {
            // :192-209 resets no DSP state: an unchanged format keeps the handle and takes the configuration's values
            // (tuning truncated to the int the configuration holds, as :195 reads it) without the action's dmMaxCorr = 0
            HipLiveControl.bpskReconfigure(handle, newTuning, newFFT ? 1 : 0, newUp ? 1 : 0);
            tuning = newTuning;
            doFFT = newFFT;
            doUp = newUp;
            if (aud != audio) {
                audio.remHandler(this);
                audio.remRawHandler(this);
                audio = aud;
                if (rawPath)
                    audio.addRawHandler(this);
                else
                    audio.addHandler(this);
            }
            return;
        }
        if (audio != null) {
            audio.remHandler(this);
            audio.remRawHandler(this);
        }
        audio = aud;
        audioDesc = ad;
        tuning = newTuning;
        doFFT = newFFT;
        doUp = newUp;
        long old = handle;
        handle = 0;  // bpskCreate throws when it fails (a frame FFT-acquire mode does not support, no device memory):
                     // the freed pointer must not stay behind for a later getter, close() or setup()
        if (old != 0)
            HipNative.bpskDestroy(old);
        handle = HipNative.bpskCreate(ad.rate, ad.blen / ad.size, (int) tuning, doFFT ? 1 : 0, doUp ? 1 : 0);
        if (rawPath)
            audio.addRawHandler(this);
        else
            audio.addHandler(this);
    }

    private static boolean sameFormat(AudioDescriptor a, AudioDescriptor b) {
        return b != null && a.rate == b.rate && a.blen == b.blen && a.size == b.size && a.chns == b.chns && a.bits == b.bits;
    }

    public synchronized void receive(float[] buf) {
        HipNative.bpskReceive(handle, buf);
        afterFrame();
    }

    public synchronized void receive(byte[] raw) {
        HipNative.bpskReceiveRaw(handle, raw, audio.getICorrection(), audio.getQCorrection());
        afterFrame();
    }

    private void afterFrame() {
        int centre;
        synchronized (resultLock) {
            HipNative.bpskSnapshot(handle, counters, state, decoded, bits);
            centre = counters[9];
        }
        if (doFFT) {  // :455-456
            publish.setPublish(name + "-bpsk-tune", -1);
            publish.setPublish(name + "-bpsk-centre", centre);
        } else {      // :377-378
            publish.setPublish(name + "-bpsk-centre", -1);
            publish.setPublish(name + "-bpsk-tune", (int) tuning);
        }
        repaint();
    }

    public void hotKey(char c) {
    }

    /** the statistics of FUNcubeBPSKDemod.java:220-228 and, after a successful decode, the frame's bytes as :331-337
     *  prints them.  From the getters: takes resultLock only, never the receive() monitor. */
    public void paintComponent(Graphics g) {
        if (!isVisible())
            return;
        int[] c = getCounters();
        double[] st = getState();
        byte[] dec = getDecoded();
        g.setColor(Color.BLACK);
        g.fillRect(0, 0, getWidth(), getHeight());
        g.setColor(Color.GREEN);
        g.drawString("decodeOK=" + (c[8] != 0) + " dmErrBits=" + c[5] + " raw=" + c[0] + " ds=" + c[1] + " bit=" + c[2]
                     + " fec=" + c[3] + " dec=" + c[4], 10, 20);
        if (doFFT)
            g.drawString("centreBin=" + c[9], getWidth() - 250, 20);
        else
            g.drawString("tuning=" + tuning, getWidth() - 250, 20);
        g.drawString("e1=" + st[4], getWidth() - 250, 36);
        g.drawString("e2=" + st[5], getWidth() - 250, 52);
        g.drawString("eO=" + st[3], getWidth() - 250, 68);
        g.drawString("com=" + c[7] + " co=" + c[6], getWidth() - 250, 84);
        if (c[8] != 0) {
            for (int n = 0; n < dec.length; n += 16)
                for (int l = 0; l < 16 && n + l < dec.length; l++)
                    g.drawString(String.format("%02x ", dec[n + l] & 0xff), 10 + (20 * l), 40 + n);
        }
    }

    // The getters below serve the painting thread (FUNcubeBPSKDemod.java:220-228,331-337).  They take only resultLock,
    // never this object's monitor, which the audio thread holds for the whole of receive(): a repaint never waits for
    // the GPU, and never delays the audio loop.

    /** cntRaw,cntDS,cntBit,cntFEC,cntDec,dmErrBits,dmCorr,dmMaxCorr,decodeOK,centreBin */
    public int[] getCounters() {
        synchronized (resultLock) {
            return java.util.Arrays.copyOf(counters, 10);
        }
    }

    public boolean isDecodeOK() {
        synchronized (resultLock) {
            return counters[8] != 0;
        }
    }

    /** decoded[] (:111): the last successfully decoded frame */
    public byte[] getDecoded() {
        synchronized (resultLock) {
            return decoded.clone();
        }
    }

    /** bits sliced during the last frame, +1/-1 -- the first 512 of them (a 2048-sample frame slices about 25, the
     *  default 9600-sample frame 120; getAllBits() has no such limit) */
    public byte[] getBits() {
        synchronized (resultLock) {
            return java.util.Arrays.copyOf(bits, Math.min(counters[10], bits.length));
        }
    }

    /** every bit of the last frame whatever its size; a device call, so it takes the receive() monitor: for the audio
     *  thread or a test, not for the painter */
    public synchronized byte[] getAllBits() {
        int n;
        synchronized (resultLock) {
            n = counters[10];
        }
        byte[] out = new byte[Math.max(n, 1)];
        int got = HipNative.bpskBits(handle, out);
        return java.util.Arrays.copyOf(out, Math.max(0, Math.min(got, out.length)));
    }

    /** tuPhase,vcoPhase,dmBitPhase,dmEnergyOut,energy1,energy2,avePeakPower,aveCentreBin,dmEnergy[8],dmLastIQ[2] */
    public double[] getState() {
        synchronized (resultLock) {
            return state.clone();
        }
    }

    public synchronized void close() {
        if (audio != null) {
            audio.remHandler(this);
            audio.remRawHandler(this);
        }
        publish.unlisten(this);
        long old = handle;
        handle = 0;
        if (old != 0)
            HipNative.bpskDestroy(old);
        logger.statusMsg(name + ": closed");
    }
}
