// embed_common.h -- what the two embedding units (batch_embed.hip: float bag-of-words rows; batch_embed_idx.hip: word
// indices) share on the host.
#pragma once
#include "hops_common.h"

namespace {

// formats of a hop's memory bytes from the net: values on act[h]; keys on att[h] -- except mode 3 with a finer weight grid,
// whose keys keep the weight grid (qfmt.h::ham_key_format) -- and the hops whose keys follow the minus-zero rule
template <typename Args>
static void fill_key_formats(Args &a, const qmann_net *net)
{
    a.key_mz = 0;
    for (uint32_t h = 0; h < net->n_hop; h++) {
        a.act[h] = qm_qfmt(net->act[h]);
        a.w[h] = qm_qfmt(net->w[h]);
        bool mz = false;
        a.att[h] = ham_key_format(net->attention_mode, qm_qfmt(h == 0 ? net->w[0] : net->act[h - 1]), a.w[h], qm_qfmt(net->att[h]), &mz);
        if (mz) a.key_mz |= 1u << h;
    }
}

}  // namespace
