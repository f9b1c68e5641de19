/* oracle/ref/rtl-sdr.h -- TEST INFRASTRUCTURE, not product code.
 *
 * Declarations only, written for this repository: the handful of librtlsdr entry points
 * that the reference's jonti/sdr.cpp and sdrj.cpp name, so that those two files compile
 * unmodified into the sdrj oracle (oracle/ref/Makefile, libsdrjref*.so).  No librtlsdr
 * code or header is involved.  oracle/ref/sdrj_harness.cpp defines every function below
 * as a stub that fails: the oracle never talks to a dongle, it feeds bytes itself.
 */
#ifndef SDRX_ORACLE_RTL_SDR_H
#define SDRX_ORACLE_RTL_SDR_H

#include <stdint.h>

typedef struct rtlsdr_dev rtlsdr_dev_t;
typedef void (*rtlsdr_read_async_cb_t)(unsigned char *buf, uint32_t len, void *ctx);

uint32_t rtlsdr_get_device_count(void);
const char *rtlsdr_get_device_name(uint32_t index);
int rtlsdr_get_device_usb_strings(uint32_t index, char *manufact, char *product, char *serial);
int rtlsdr_get_index_by_serial(const char *serial);
int rtlsdr_open(rtlsdr_dev_t **dev, uint32_t index);
int rtlsdr_close(rtlsdr_dev_t *dev);
int rtlsdr_set_center_freq(rtlsdr_dev_t *dev, uint32_t freq);
int rtlsdr_set_tuner_gain_mode(rtlsdr_dev_t *dev, int manual);
int rtlsdr_set_tuner_gain(rtlsdr_dev_t *dev, int gain);
int rtlsdr_set_sample_rate(rtlsdr_dev_t *dev, uint32_t rate);
int rtlsdr_set_agc_mode(rtlsdr_dev_t *dev, int on);
int rtlsdr_set_bias_tee(rtlsdr_dev_t *dev, int on);
int rtlsdr_reset_buffer(rtlsdr_dev_t *dev);
int rtlsdr_read_async(rtlsdr_dev_t *dev, rtlsdr_read_async_cb_t cb, void *ctx, uint32_t buf_num, uint32_t buf_len);
int rtlsdr_cancel_async(rtlsdr_dev_t *dev);

#endif
