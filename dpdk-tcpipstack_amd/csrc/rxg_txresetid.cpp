// rxg_txresetid.cpp — rxg_reset_set_id: a prebuilt reset (rxg_tx_reset_dev) given another
// packet_id.  Pure host code (rxg.h and libc only: it compiles stand-alone).
#include "rxg.h"

extern "C" void rxg_reset_set_id(uint8_t *f, uint16_t ip_id)
{
    if (!f) return;
    f[18] = (uint8_t)(ip_id & 0xFFu);  // packet_id as it stands (ip.c:106)
    f[19] = (uint8_t)(ip_id >> 8);
    f[24] = f[25] = 0;                 // hdr_checksum = 0 while summing (ip.c:102)
    // calculate_checksum(hdr, 20) (ip.c:44-59): big-endian 16-bit words, folded, complemented
    uint32_t sum = 0;
    for (int i = 0; i < 20; i += 2) sum += ((uint32_t)f[14 + i] << 8) | f[15 + i];
    while (sum & 0xFFFF0000u) sum = (sum & 0xFFFFu) + (sum >> 16);
    const uint16_t ck = (uint16_t)~sum;
    f[24] = (uint8_t)(ck >> 8);        // stored htons (ip.c:107)
    f[25] = (uint8_t)(ck & 0xFFu);
}
