{-# LANGUAGE ForeignFunctionInterface #-}
-- | Raw bindings of libtextcomp.so (include/textcomp.h).  NOT COMPILED IN THIS REPOSITORY'S
-- PIPELINE: the build image has no GHC; the same C ABI is exercised by the C++ and Python
-- mirrors and their parity tests.  Every import is `safe`: device calls run for milliseconds.
module Data.TextCompression.FFI where

import Data.Int (Int16, Int32, Int64)
import Data.Word (Word16, Word32, Word64, Word8)
import Foreign.C.String (CString)
import Foreign.Ptr (Ptr)

data TcCtx
data TcFm
data TcComm

foreign import ccall safe "tc_ctx_create"  c_tc_ctx_create  :: Int32 -> Ptr (Ptr TcCtx) -> IO Int32
foreign import ccall safe "tc_ctx_destroy" c_tc_ctx_destroy :: Ptr TcCtx -> IO ()
foreign import ccall safe "tc_last_error"  c_tc_last_error  :: Ptr TcCtx -> IO CString

-- Data.BWT
foreign import ccall safe "tc_bwt_encode"
  c_tc_bwt_encode :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_bwt_decode_sym"
  c_tc_bwt_decode_sym :: Ptr TcCtx -> Ptr Int16 -> Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_suffix_array"
  c_tc_suffix_array :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word32 -> IO Int32
-- the enhanced suffix array (no counterpart in the reference): the suffix array with text and array in HBM, the LCP
-- array that goes with it (n + 1 entries, lcp[0] = 0; the host form's sa may be nullPtr), and one reduction over an
-- LCP array in HBM: largest entry, smallest row holding it, sum
foreign import ccall safe "tc_suffix_array_dev"
  c_tc_suffix_array_dev :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word32 -> IO Int32
foreign import ccall safe "tc_lcp_array_dev"
  c_tc_lcp_array_dev :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word32 -> Ptr Word32 -> IO Int32
foreign import ccall safe "tc_lcp_array"
  c_tc_lcp_array :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word32 -> Ptr Word32 -> IO Int32
foreign import ccall safe "tc_lcp_summary_dev"
  c_tc_lcp_summary_dev :: Ptr TcCtx -> Ptr Word32 -> Word64 -> Ptr Word32 -> Ptr Word64 -> Ptr Word64 -> IO Int32
-- Data.MTF
foreign import ccall safe "tc_mtf_encode_sym"
  c_tc_mtf_encode_sym :: Ptr TcCtx -> Ptr Int16 -> Word64 -> Ptr Word16 -> Ptr Int16 -> Ptr Word32 -> IO Int32
foreign import ccall safe "tc_mtf_decode"
  c_tc_mtf_decode :: Ptr TcCtx -> Ptr Word16 -> Word64 -> Ptr Int16 -> Word32 -> Ptr Int16 -> IO Int32
-- Data.RLE
foreign import ccall safe "tc_rle_encode_sym"
  c_tc_rle_encode_sym :: Ptr TcCtx -> Ptr Int16 -> Word64 -> Ptr Word32 -> Ptr Int16 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_rle_decode"
  c_tc_rle_decode :: Ptr TcCtx -> Ptr Word32 -> Ptr Int16 -> Word64 -> Ptr Int16 -> Ptr Word64 -> IO Int32
-- Data.FMIndex
foreign import ccall safe "tc_fm_build"
  c_tc_fm_build :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr (Ptr TcFm) -> IO Int32
foreign import ccall safe "tc_fm_count"
  c_tc_fm_count :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Ptr Int64 -> IO Int32
foreign import ccall safe "tc_fm_free" c_tc_fm_free :: Ptr TcFm -> IO ()
foreign import ccall safe "tc_fm_locate"
  c_tc_fm_locate :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Ptr Word64 -> Ptr Word64 -> Ptr Word64 -> IO Int32
foreign import ccall unsafe "tc_fm_info"
  c_tc_fm_info :: Ptr TcFm -> Ptr Word64 -> Ptr Word32 -> Ptr Int16 -> Ptr Word64 -> Ptr Word64 -> IO Int32
-- the index with a sampled suffix array (sa_rate: a power of two up to 4096; 1 = tc_fm_build) and locate with
-- patterns and hits in device memory (no counterpart in the reference)
foreign import ccall safe "tc_fm_build_sampled"
  c_tc_fm_build_sampled :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Word32 -> Ptr (Ptr TcFm) -> IO Int32
foreign import ccall safe "tc_fm_build_sampled_dev"
  c_tc_fm_build_sampled_dev :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Word32 -> Ptr (Ptr TcFm) -> IO Int32
foreign import ccall unsafe "tc_fm_sa_rate" c_tc_fm_sa_rate :: Ptr TcFm -> Word32
foreign import ccall unsafe "tc_fm_device_bytes"
  c_tc_fm_device_bytes :: Ptr TcFm -> Int32 -> Word64
foreign import ccall safe "tc_fm_locate_dev"
  c_tc_fm_locate_dev :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Ptr Word64 -> Ptr Word64 -> Ptr Word64 -> IO Int32
-- the index with text samples (text_rate: a power of two up to 4096) and extract: the text ranges (1-based start, length)
-- read back from the index (no counterpart in the reference)
foreign import ccall safe "tc_fm_build_self"
  c_tc_fm_build_self :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Word32 -> Word32 -> Ptr (Ptr TcFm) -> IO Int32
foreign import ccall safe "tc_fm_build_self_dev"
  c_tc_fm_build_self_dev :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Word32 -> Word32 -> Ptr (Ptr TcFm) -> IO Int32
foreign import ccall unsafe "tc_fm_text_rate" c_tc_fm_text_rate :: Ptr TcFm -> Word32
foreign import ccall safe "tc_fm_extract"
  c_tc_fm_extract :: Ptr TcCtx -> Ptr TcFm -> Ptr Word64 -> Ptr Word64 -> Word64 -> Ptr Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_fm_extract_dev"
  c_tc_fm_extract_dev :: Ptr TcCtx -> Ptr TcFm -> Ptr Word64 -> Ptr Word64 -> Word64 -> Ptr Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
-- search with mismatches: count / locate within Hamming distance k (substitutions only, k at most 3; no counterpart in
-- the reference).  locate also answers each hit's distance (Ptr Word8, may be nullPtr)
foreign import ccall safe "tc_fm_count_mm"
  c_tc_fm_count_mm :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Word32 -> Ptr Int64 -> IO Int32
foreign import ccall safe "tc_fm_count_mm_dev"
  c_tc_fm_count_mm_dev :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Word32 -> Ptr Int64 -> IO Int32
foreign import ccall safe "tc_fm_locate_mm"
  c_tc_fm_locate_mm :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Word32 -> Ptr Word64 -> Ptr Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_fm_locate_mm_dev"
  c_tc_fm_locate_mm_dev :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Word32 -> Ptr Word64 -> Ptr Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
-- factorize: the greedy right-to-left longest-match parse of patterns against the text -- factor offsets, (position,
-- length) per factor, a literal is (byte, 0) -- and its inverse on an index with text samples (no counterpart in the
-- reference).  fac_pos = fac_len = nullPtr with capacity 0 asks for the sizes alone
foreign import ccall safe "tc_fm_factorize"
  c_tc_fm_factorize :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Ptr Word64 -> Ptr Word64 -> Ptr Word32 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_fm_factorize_dev"
  c_tc_fm_factorize_dev :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Ptr Word64 -> Ptr Word64 -> Ptr Word32 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_fm_unfactorize"
  c_tc_fm_unfactorize :: Ptr TcCtx -> Ptr TcFm -> Ptr Word64 -> Ptr Word64 -> Ptr Word32 -> Word64 -> Ptr Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_fm_unfactorize_dev"
  c_tc_fm_unfactorize_dev :: Ptr TcCtx -> Ptr TcFm -> Ptr Word64 -> Ptr Word64 -> Ptr Word32 -> Word64 -> Ptr Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
-- matching statistics and maximal exact matches on an index with the LCP part (tc_fm_build_lcp: sa_rate, then text_rate
-- or 0; no counterpart in the reference): per pattern position the longest match's length, first-row position and
-- occurrences (the last two may be nullPtr); the MEMs as offsets and (start, position, length), the three nullPtr with
-- capacity 0 asks for the sizes alone
foreign import ccall safe "tc_fm_build_lcp"
  c_tc_fm_build_lcp :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Word32 -> Word32 -> Ptr (Ptr TcFm) -> IO Int32
foreign import ccall safe "tc_fm_build_lcp_dev"
  c_tc_fm_build_lcp_dev :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Word32 -> Word32 -> Ptr (Ptr TcFm) -> IO Int32
foreign import ccall unsafe "tc_fm_has_lcp" c_tc_fm_has_lcp :: Ptr TcFm -> Int32
foreign import ccall safe "tc_fm_match_stats"
  c_tc_fm_match_stats :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Ptr Word32 -> Ptr Word64 -> Ptr Word32 -> IO Int32
foreign import ccall safe "tc_fm_match_stats_dev"
  c_tc_fm_match_stats_dev :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Ptr Word32 -> Ptr Word64 -> Ptr Word32 -> IO Int32
foreign import ccall safe "tc_fm_mems"
  c_tc_fm_mems :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Word32 -> Ptr Word64 -> Ptr Word64 -> Ptr Word64 -> Ptr Word32 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_fm_mems_dev"
  c_tc_fm_mems_dev :: Ptr TcCtx -> Ptr TcFm -> Ptr Word8 -> Ptr Word64 -> Word64 -> Word32 -> Ptr Word64 -> Ptr Word64 -> Ptr Word64 -> Ptr Word32 -> Ptr Word64 -> IO Int32
-- stored / shipped form (no counterpart in the reference): one record, or any length cut into records
foreign import ccall unsafe "tc_container_bound"
  c_tc_container_bound :: Word64 -> Word32 -> Word64
foreign import ccall safe "tc_encode_container"
  c_tc_encode_container :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_encode_container_dev"
  c_tc_encode_container_dev :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
foreign import ccall unsafe "tc_ctx_set_container_coding"
  c_tc_ctx_set_container_coding :: Ptr TcCtx -> Int32 -> IO Int32
foreign import ccall unsafe "tc_ctx_get_container_coding"
  c_tc_ctx_get_container_coding :: Ptr TcCtx -> IO Int32
foreign import ccall unsafe "tc_container_coding"
  c_tc_container_coding :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Int32 -> IO Int32
foreign import ccall safe "tc_container_info"
  c_tc_container_info :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word64 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_decode_container"
  c_tc_decode_container :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
foreign import ccall unsafe "tc_stream_bound"
  c_tc_stream_bound :: Word64 -> Word64 -> Word64
foreign import ccall safe "tc_encode_stream"
  c_tc_encode_stream :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_stream_info"
  c_tc_stream_info :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word64 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_decode_stream"
  c_tc_decode_stream :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr Word8 -> Ptr Word64 -> IO Int32
-- the exchange of the multi-GPU path (one process per GPU; include/textcomp.h, tc_comm_*)
foreign import ccall safe "tc_comm_unique_id"
  c_tc_comm_unique_id :: Ptr TcCtx -> Ptr Word8 -> IO Int32
foreign import ccall safe "tc_comm_create"
  c_tc_comm_create :: Ptr TcCtx -> Ptr Word8 -> Int32 -> Int32 -> Ptr (Ptr TcComm) -> IO Int32
foreign import ccall safe "tc_comm_destroy" c_tc_comm_destroy :: Ptr TcComm -> IO ()
foreign import ccall safe "tc_comm_gather"
  c_tc_comm_gather :: Ptr TcComm -> Int32 -> Ptr Word8 -> Word64 -> Ptr Word8 -> Word64 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_comm_wait" c_tc_comm_wait :: Ptr TcComm -> IO Int32
foreign import ccall safe "tc_comm_broadcast"
  c_tc_comm_broadcast :: Ptr TcComm -> Int32 -> Ptr Word8 -> Word64 -> IO Int32
foreign import ccall unsafe "tc_fm_export_bound"
  c_tc_fm_export_bound :: Ptr TcFm -> Int32 -> Word64
foreign import ccall safe "tc_fm_export_dev"
  c_tc_fm_export_dev :: Ptr TcCtx -> Ptr TcFm -> Int32 -> Ptr Word8 -> Ptr Word64 -> IO Int32
foreign import ccall safe "tc_fm_import_dev"
  c_tc_fm_import_dev :: Ptr TcCtx -> Ptr Word8 -> Word64 -> Ptr (Ptr TcFm) -> IO Int32
