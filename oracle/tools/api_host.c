/* TEST INFRASTRUCTURE (tests/test_host_logic.py::test_program_written_against_the_reference_header_links): a host program written
 * against the REFERENCE's own public header that calls one function of every family of its API.  oracle/Makefile compiles it to
 * oracle/_ref/api_host.o with -Wall -Werror against that header where it lies; the test links the object against
 * libmbe_neo_amd.so. */
#include <mbelib-neo/mbelib.h>
int main(void) {
    static mbe_parms cur, prev, enh;
    static char imbe_fr[8][23], imbe7100_fr[7][24], ambe_fr[4][24], imbe_d[88], ambe_d[49];
    static mbe_soft_bit soft_i[8][23], soft_a[4][24];
    static short pcm[160];
    static float pcmf[160];
    mbe_process_result res;
    long block = 0;
    mbe_initMbeParms(&cur, &prev, &enh);
    mbe_initProcessResult(&res);
    mbe_setThreadRngSeed(1u);
    int n = 0;
    n += mbe_eccImbe7200x4400C0(imbe_fr) + mbe_demodulateImbe7200x4400Data(imbe_fr) + mbe_eccImbe7200x4400Data(imbe_fr, imbe_d);
    n += mbe_decodeImbe4400Parms(imbe_d, &cur, &prev);
    n += mbe_processImbe7200x4400Frame(pcm, &res, (const char(*)[23])imbe_fr, imbe_d, &cur, &prev, &enh);
    n += mbe_processImbe7200x4400SoftFramef(pcmf, &res, (const mbe_soft_bit(*)[23])soft_i, imbe_d, &cur, &prev, &enh);
    n += mbe_processImbe7100x4400Framef(pcmf, &res, (const char(*)[24])imbe7100_fr, imbe_d, &cur, &prev, &enh);
    n += mbe_convertImbe7100to7200(imbe_d);
    n += mbe_processAmbe3600x2450Frame(pcm, &res, (const char(*)[24])ambe_fr, ambe_d, &cur, &prev, &enh);
    n += mbe_processAmbe3600x2450SoftFrame(pcm, &res, (const mbe_soft_bit(*)[24])soft_a, ambe_d, &cur, &prev, &enh);
    n += mbe_processAmbe3600x2400Framef(pcmf, &res, (const char(*)[24])ambe_fr, ambe_d, &cur, &prev, &enh);
    n += mbe_decodeAmbe2450Parms(ambe_d, &cur, &prev) + mbe_decodeAmbe2400Parms(ambe_d, &cur, &prev);
    n += mbe_eccAmbe3600x2450C0(ambe_fr) + mbe_demodulateAmbe3600x2400Data(ambe_fr);
    n += mbe_checkGolayBlock(&block) + mbe_golay2312(imbe_fr[0], imbe_fr[1]) + mbe_hamming1511(imbe_fr[4], imbe_fr[5]);
    mbe_synthesizeSpeechf(pcmf, &cur, &prev);
    mbe_spectralAmpEnhance(&cur);
    mbe_applyAdaptiveSmoothing(&cur, &prev);
    mbe_floattoshort(pcmf, pcm);
    mbe_synthesizeComfortNoise(pcm);
    mbe_synthesizeTonef(pcmf, ambe_d, &cur);
    mbe_dumpImbe7200x4400Frame((const char(*)[23])imbe_fr);
    return n + (mbe_versionString() != 0);
}
