"""Channel coding on MI355X -- same public names as /root/reference/commpy/channelcoding/__init__.py:65-71
for the decoding hot path (Viterbi, BCJR/turbo, LDPC BP) and the host-side code descriptions around it."""
from commpy_amd.channelcoding.convcode import (Trellis, conv_encode, conv_encode_batch, viterbi_decode, puncturing,
                                               depuncturing)
from commpy_amd.channelcoding.interleavers import RandInterlv
from commpy_amd.channelcoding.turbo import turbo_encode, map_decode, turbo_decode
from commpy_amd.channelcoding.ldpc import (build_matrix, get_ldpc_code_params, ldpc_bp_decode, write_ldpc_params,
                                           triang_ldpc_systematic_encode)
from commpy_amd.channelcoding.polar import (polar_reliability_order, PolarCode, crc_append, crc_check, polar_encode,
                                            polar_decode)
from commpy_amd.channelcoding.gfields import GF, polydivide, polymultiply, poly_to_string
from commpy_amd.channelcoding.algcode import cyclic_code_genpoly, bch_genpoly, rs_genpoly
from commpy_amd.channelcoding.bch import BCHCode, bch_encode, bch_decode, chase_decode
from commpy_amd.channelcoding.productcode import ProductCode, tpc_encode, tpc_decode
from commpy_amd.channelcoding.rs import RSCode, rs_encode, rs_decode
from commpy_amd.channelcoding.tailbiting import tailbiting_encode, tailbiting_decode
from commpy_amd.channelcoding.ldpc_layered import ldpc_layers, ldpc_layered_decode

__all__ = ['Trellis', 'conv_encode', 'conv_encode_batch', 'viterbi_decode', 'puncturing', 'depuncturing',
           'RandInterlv', 'turbo_encode', 'map_decode', 'turbo_decode', 'build_matrix', 'get_ldpc_code_params',
           'ldpc_bp_decode', 'write_ldpc_params', 'triang_ldpc_systematic_encode',
           'polar_reliability_order', 'PolarCode', 'crc_append', 'crc_check', 'polar_encode', 'polar_decode',
           'GF', 'polydivide', 'polymultiply', 'poly_to_string', 'cyclic_code_genpoly', 'bch_genpoly', 'BCHCode', 'bch_encode',
           'bch_decode', 'rs_genpoly', 'RSCode', 'rs_encode', 'rs_decode', 'tailbiting_encode', 'tailbiting_decode',
           'ldpc_layers', 'ldpc_layered_decode', 'chase_decode', 'ProductCode', 'tpc_encode', 'tpc_decode']
