// hxcpp externs over include/jsplayer_amd.h — one row per export the three classes below use.
// Build: add  <files id="haxe"> <compilerflag value="-I${JSPLAYER_AMD}/include"/> </files>
//             <target id="haxe"> <lib name="-L${JSPLAYER_AMD}/jsplayer_amd"/> <lib name="-ljsplayer_amd"/> </target>
// to the project's Build.xml (or keep the @:buildXml below and set JSPLAYER_AMD in the environment).
#if cpp
package;

import cpp.ConstCharStar;
import cpp.RawConstPointer;
import cpp.RawPointer;
import cpp.SizeT;
import cpp.UInt64;
import cpp.UInt8;

@:keep
@:include("jsplayer_amd.h")
@:buildXml('
<files id="haxe"><compilerflag value="-I${JSPLAYER_AMD}/include"/></files>
<target id="haxe"><lib name="-L${JSPLAYER_AMD}/jsplayer_amd"/><lib name="-ljsplayer_amd"/></target>
')
extern class JspNative {
    // IVideoCodec.hx:16-29 <-> C ABI, see INTEGRATION.md §1
    @:native("jsp_codec_create")       static function create(kind:Int, w:Int, h:Int, bpp:Int, palette:RawConstPointer<UInt8>, paletteBytes:Int, device:Int):RawPointer<JspCodec>;
    @:native("jsp_codec_destroy")      static function destroy(c:RawPointer<JspCodec>):Void;
    @:native("jsp_preinit")            static function preinit(c:RawPointer<JspCodec>, lines:Int):Int;
    @:native("jsp_previous_frame")     static function previousFrame(c:RawPointer<JspCodec>):RawPointer<cpp.Int32>;
    @:native("jsp_is_key_frame")       static function isKeyFrame(c:RawPointer<JspCodec>, src:RawConstPointer<UInt8>, n:SizeT):Int;
    @:native("jsp_state")              static function state(c:RawPointer<JspCodec>):Int;
    @:native("jsp_continue_i")         static function continueI(c:RawPointer<JspCodec>):Int;
    @:native("jsp_decompress_i")       static function decompressI(c:RawPointer<JspCodec>, src:RawConstPointer<UInt8>, n:SizeT, dst:RawPointer<cpp.Int32>):Int;
    @:native("jsp_decompress_p")       static function decompressP(c:RawPointer<JspCodec>, src:RawConstPointer<UInt8>, n:SizeT, dst:RawPointer<cpp.Int32>,
                                                                   dataPnt:RawPointer<RawPointer<cpp.Int32>>, significant:RawPointer<Int>):Int;
    @:native("jsp_needs_index")        static function needsIndex(c:RawPointer<JspCodec>):Int;
    @:native("jsp_last_error")         static function lastError():ConstCharStar;
    @:native("jsp_set_option")         static function setOption(c:RawPointer<JspCodec>, key:ConstCharStar, value:ConstCharStar):Int;
    @:native("jsp_counter")            static function counter(c:RawPointer<JspCodec>, name:ConstCharStar):cpp.Int64;   // diagnostics: "async_reruns", "lookback_fallbacks"
    // the asynchronous form of DecompressI / DecompressP (optional: a Manager that decodes ahead of display)
    @:native("jsp_decompress_i_async") static function decompressIAsync(c:RawPointer<JspCodec>, src:RawConstPointer<UInt8>, n:SizeT, dst:RawPointer<cpp.Int32>, ticket:RawPointer<UInt64>):Int;
    @:native("jsp_decompress_p_async") static function decompressPAsync(c:RawPointer<JspCodec>, src:RawConstPointer<UInt8>, n:SizeT, dst:RawPointer<cpp.Int32>, ticket:RawPointer<UInt64>):Int;
    @:native("jsp_prefetch")           static function prefetch(c:RawPointer<JspCodec>, host:RawConstPointer<UInt8>, bytes:SizeT):Int;   // a stretch of the file ahead of the frames submitted next: one copy instead of one per frame
    @:native("jsp_wait")               static function wait(c:RawPointer<JspCodec>, ticket:UInt64, dataPnt:RawPointer<RawPointer<cpp.Int32>>, significant:RawPointer<Int>):Int;
    // the seek branch of Manager.GetDecompressedFrame (Manager.hx:216-259), MSVideo1: frames from the nearest key frame up to the target, composed into `dst` in one call
    @:native("jsp_seek")               static function seek(c:RawPointer<JspCodec>, nframes:Int, srcs:RawPointer<RawConstPointer<UInt8>>, lens:RawPointer<SizeT>,
                                                            isKey:RawConstPointer<UInt8>, dst:RawPointer<cpp.Int32>,
                                                            dataPnt:RawPointer<RawPointer<cpp.Int32>>, significant:RawPointer<Int>):Int;
    // Manager.SkipStills over DataLoader.FindPossibleChange (Manager.hx:289-317), MSVideo1: the first frame from `first` on that changes the picture, composed into `dst` in one call
    @:native("jsp_find_change")        static function findChange(c:RawPointer<JspCodec>, nframes:Int, srcs:RawPointer<RawConstPointer<UInt8>>, lens:RawPointer<SizeT>,
                                                                  isKey:RawConstPointer<UInt8>, first:Int, keyBefore:RawConstPointer<UInt8>, keyBeforeLen:SizeT,
                                                                  keyRow:Int, dst:RawPointer<cpp.Int32>, found:RawPointer<Int>, changed:RawPointer<Int>,
                                                                  significance:RawPointer<Int>, dataPnt:RawPointer<RawPointer<cpp.Int32>>):Int;
    // seek index (Main.on_prevframe / on_click, Manager.hx:184-208), MSVideo1: a range kept resident in HBM, any frame of it shown by ONE launch
    @:native("jsp_index_build")        static function indexBuild(c:RawPointer<JspCodec>, nframes:Int, srcs:RawPointer<RawConstPointer<UInt8>>, lens:RawPointer<SizeT>,
                                                                  isKey:RawConstPointer<UInt8>, keyRow:Int):RawPointer<JspIndex>;
    @:native("jsp_index_show")         static function indexShow(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, t:Int, dst:RawPointer<cpp.Int32>, adopt:Int,
                                                                 dataPnt:RawPointer<RawPointer<cpp.Int32>>, significant:RawPointer<Int>):Int;
    @:native("jsp_index_thumb_size")   static function indexThumbSize(idx:RawPointer<JspIndex>, scale:Int, width:RawPointer<Int>, height:RawPointer<Int>):Int;
    @:native("jsp_index_thumbs")       static function indexThumbs(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, n:Int, frames:RawConstPointer<Int>, scale:Int, cols:Int,
                                                                   out:RawPointer<cpp.Int32>, outPixels:SizeT):Int;
    @:native("jsp_index_present")      static function indexPresent(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, n:Int, frames:RawConstPointer<Int>,
                                                                    out:RawPointer<cpp.Int32>, outInts:SizeT, winW:Int, winH:Int, outPitch:SizeT, cols:Int,
                                                                    k:Float, dx:Float, dy:Float, mode:Int, filter:Int, background:cpp.UInt32):Int;
    @:native("jsp_index_tensor")       static function indexTensor(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, n:Int, frames:RawConstPointer<Int>,
                                                                   out:RawPointer<cpp.Void>, outBytes:SizeT, winW:Int, winH:Int,
                                                                   k:Float, dx:Float, dy:Float, mode:Int, filter:Int, background:cpp.UInt32,
                                                                   dtype:Int, layout:Int, scale:RawConstPointer<cpp.Float32>, bias:RawConstPointer<cpp.Float32>):Int;
    @:native("jsp_index_play")         static function indexPlay(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, first:Int, n:Int, stride:Int,
                                                                 dsts:RawPointer<RawPointer<cpp.Int32>>, adoptK:Int,
                                                                 dataPnts:RawPointer<RawPointer<cpp.Int32>>, significant:RawPointer<Int>):Int;
    @:native("jsp_index_activity_size") static function indexActivitySize(idx:RawPointer<JspIndex>, cols:RawPointer<Int>, rows:RawPointer<Int>):Int;
    @:native("jsp_index_activity")     static function indexActivity(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, first:Int, n:Int,
                                                                     out:RawPointer<cpp.UInt16>, outElems:SizeT):Int;
    // refFrame -1 .. nframes-1 with refPicture null, or JSP_REF_PICTURE (-2) with a device picture of X * Y words
    @:native("jsp_index_distance")     static function indexDistance(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, refFrame:Int,
                                                                     refPicture:RawConstPointer<cpp.Int32>, first:Int, n:Int,
                                                                     out:RawPointer<cpp.UInt16>, outElems:SizeT):Int;
    @:native("jsp_index_key_frame_bound") static function indexKeyFrameBound(idx:RawPointer<JspIndex>, bytes:RawPointer<SizeT>):Int;
    @:native("jsp_index_key_frame")    static function indexKeyFrame(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, t:Int, out:RawPointer<UInt8>,
                                                                     cap:SizeT, len:RawPointer<SizeT>):Int;
    @:native("jsp_index_delta_bound")  static function indexDeltaBound(idx:RawPointer<JspIndex>, bytes:RawPointer<SizeT>):Int;
    @:native("jsp_index_delta_frames") static function indexDeltaFrames(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, n:Int, from:RawConstPointer<Int>,
                                                                        to:RawConstPointer<Int>, out:RawPointer<UInt8>, cap:SizeT,
                                                                        lens:RawPointer<SizeT>, total:RawPointer<SizeT>):Int;
    @:native("jsp_index_tight_frames") static function indexTightFrames(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, n:Int, from:RawConstPointer<Int>,
                                                                        to:RawConstPointer<Int>, out:RawPointer<UInt8>, cap:SizeT,
                                                                        lens:RawPointer<SizeT>, total:RawPointer<SizeT>):Int;
    // the frames of a block rectangle (bx, by, bw, bh; table order): from = CROP_KEY makes a key pair, flags = CROP_TIGHT the tight rule; keys may be null
    static inline var CROP_KEY:Int = -2;
    static inline var CROP_TIGHT:Int = 1;
    @:native("jsp_index_crop_bound")   static function indexCropBound(idx:RawPointer<JspIndex>, bw:Int, bh:Int, bytes:RawPointer<SizeT>):Int;
    @:native("jsp_index_crop_frames")  static function indexCropFrames(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, bx:Int, by:Int, bw:Int, bh:Int,
                                                                       n:Int, from:RawConstPointer<Int>, to:RawConstPointer<Int>, flags:Int,
                                                                       out:RawPointer<UInt8>, cap:SizeT, lens:RawPointer<SizeT>, keys:RawPointer<Int>,
                                                                       total:RawPointer<SizeT>):Int;
    // the same for a rectangle of bw x bh blocks that moves: per pair its origin (x, y) at `from` (fromXy, not read for key pairs) and at `to` (toXy)
    @:native("jsp_index_pan_frames")   static function indexPanFrames(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, bw:Int, bh:Int, n:Int,
                                                                      from:RawConstPointer<Int>, to:RawConstPointer<Int>, fromXy:RawConstPointer<Int>,
                                                                      toXy:RawConstPointer<Int>, flags:Int, out:RawPointer<UInt8>, cap:SizeT,
                                                                      lens:RawPointer<SizeT>, keys:RawPointer<Int>, total:RawPointer<SizeT>):Int;
    // the same for a rectangle that stands, with pairs in either direction: from > to steps back, from == to holds (a reversed clip, a boomerang)
    @:native("jsp_index_path_frames")  static function indexPathFrames(c:RawPointer<JspCodec>, idx:RawPointer<JspIndex>, bx:Int, by:Int, bw:Int, bh:Int,
                                                                       n:Int, from:RawConstPointer<Int>, to:RawConstPointer<Int>, flags:Int,
                                                                       out:RawPointer<UInt8>, cap:SizeT, lens:RawPointer<SizeT>, keys:RawPointer<Int>,
                                                                       total:RawPointer<SizeT>):Int;
    @:native("jsp_index_significance") static function indexSignificance(idx:RawPointer<JspIndex>, out:RawPointer<Int>):Int;
    @:native("jsp_index_destroy")      static function indexDestroy(idx:RawPointer<JspIndex>):Void;
    // ScreenPressor seek index: the host entropy stage over a range ONCE, its records resident in HBM, any frame of it shown by ONE launch (the codec is only lent)
    @:native("jsp_sp_index_build")        static function spIndexBuild(c:RawPointer<JspCodec>, nframes:Int, srcs:RawPointer<RawConstPointer<UInt8>>, lens:RawPointer<SizeT>,
                                                                       isKey:RawConstPointer<UInt8>, keyRow:Int):RawPointer<JspSpIndex>;
    @:native("jsp_sp_index_show")         static function spIndexShow(c:RawPointer<JspCodec>, idx:RawPointer<JspSpIndex>, t:Int, dst:RawPointer<cpp.Int32>,
                                                                      significant:RawPointer<Int>):Int;
    @:native("jsp_sp_index_thumb_size")   static function spIndexThumbSize(idx:RawPointer<JspSpIndex>, scale:Int, width:RawPointer<Int>, height:RawPointer<Int>):Int;
    @:native("jsp_sp_index_thumbs")       static function spIndexThumbs(c:RawPointer<JspCodec>, idx:RawPointer<JspSpIndex>, n:Int, frames:RawConstPointer<Int>, scale:Int, cols:Int,
                                                                        out:RawPointer<cpp.Int32>, outPixels:SizeT):Int;
    @:native("jsp_sp_index_present")      static function spIndexPresent(c:RawPointer<JspCodec>, idx:RawPointer<JspSpIndex>, n:Int, frames:RawConstPointer<Int>,
                                                                         out:RawPointer<cpp.Int32>, outInts:SizeT, winW:Int, winH:Int, outPitch:SizeT, cols:Int,
                                                                         k:Float, dx:Float, dy:Float, mode:Int, filter:Int, background:cpp.UInt32):Int;
    @:native("jsp_sp_index_tensor")       static function spIndexTensor(c:RawPointer<JspCodec>, idx:RawPointer<JspSpIndex>, n:Int, frames:RawConstPointer<Int>,
                                                                        out:RawPointer<cpp.Void>, outBytes:SizeT, winW:Int, winH:Int,
                                                                        k:Float, dx:Float, dy:Float, mode:Int, filter:Int, background:cpp.UInt32,
                                                                        dtype:Int, layout:Int, scale:RawConstPointer<cpp.Float32>, bias:RawConstPointer<cpp.Float32>):Int;
    @:native("jsp_sp_index_play")         static function spIndexPlay(c:RawPointer<JspCodec>, idx:RawPointer<JspSpIndex>, first:Int, n:Int, stride:Int,
                                                                      dsts:RawPointer<RawPointer<cpp.Int32>>, significant:RawPointer<Int>):Int;
    @:native("jsp_sp_index_activity_size") static function spIndexActivitySize(idx:RawPointer<JspSpIndex>, cols:RawPointer<Int>, rows:RawPointer<Int>):Int;
    @:native("jsp_sp_index_activity")     static function spIndexActivity(c:RawPointer<JspCodec>, idx:RawPointer<JspSpIndex>, first:Int, n:Int,
                                                                          out:RawPointer<cpp.UInt16>, outElems:SizeT):Int;
    @:native("jsp_sp_index_distance")     static function spIndexDistance(c:RawPointer<JspCodec>, idx:RawPointer<JspSpIndex>, refFrame:Int,
                                                                          refPicture:RawConstPointer<cpp.Int32>, first:Int, n:Int,
                                                                          out:RawPointer<cpp.UInt16>, outElems:SizeT):Int;
    @:native("jsp_sp_index_significance") static function spIndexSignificance(idx:RawPointer<JspSpIndex>, out:RawPointer<Int>):Int;
    @:native("jsp_sp_index_info")         static function spIndexInfo(idx:RawPointer<JspSpIndex>, nframes:RawPointer<Int>, deviceBytes:RawPointer<cpp.UInt64>,
                                                                      hostBytes:RawPointer<cpp.UInt64>):Int;
    @:native("jsp_sp_index_destroy")      static function spIndexDestroy(idx:RawPointer<JspSpIndex>):Void;
    // frame pool in HBM (Manager.hx:114-118) and the two Manager passes that follow the codec
    @:native("jsp_key_frame_differs")  static function keyFrameDiffers(c:RawPointer<JspCodec>):Int;
    @:native("jsp_device_count")       static function deviceCount():Int;
    @:native("jsp_assign_stream")      static function assignStream(streamIndex:Int, devices:RawPointer<Int>, ndev:Int):Int;
    @:native("jsp_reduce_counters")    static function reduceCounters(devices:RawPointer<Int>, ndev:Int, perDevice:RawPointer<cpp.UInt64>, total:RawPointer<cpp.UInt64>, viaRccl:RawPointer<Int>):Int;
    @:native("jsp_pool_create")        static function poolCreate(device:Int, w:Int, h:Int, nbuf:Int):RawPointer<JspPool>;
    @:native("jsp_pool_store_rate")    static function poolStoreRate(p:RawPointer<JspPool>, attempts:RawPointer<Int>):Float;   // diagnostics: what the placement probe of a large pool found
    @:native("jsp_pool_probe_info")    static function poolProbeInfo(p:RawPointer<JspPool>, probeMs:RawPointer<Float>, heldPeak:RawPointer<cpp.UInt64>, holdLimit:RawPointer<cpp.UInt64>):Int;
    @:native("jsp_pool_probe_rates")   static function poolProbeRates(p:RawPointer<JspPool>, rates:RawPointer<Float>, cap:Int):Int;
    @:native("jsp_pool_buffer")        static function poolBuffer(p:RawPointer<JspPool>, i:Int):RawPointer<cpp.Int32>;
    @:native("jsp_pool_destroy")       static function poolDestroy(p:RawPointer<JspPool>):Void;
    @:native("jsp_download")           static function download(deviceFrame:RawConstPointer<cpp.Int32>, host:RawPointer<cpp.Int32>, npixels:SizeT):Int;
    @:native("jsp_display_convert")    static function displayConvert(frame:RawConstPointer<cpp.Int32>, out:RawPointer<cpp.Int32>, w:Int, h:Int, mode:Int, flipRows:Int, stream:RawPointer<cpp.Void>):Int;
    // the display matrix of Main.on_stage_resize (Main.hx:301-318) and the window it shows, one launch: conversion, row flip, crop, resampling
    @:native("jsp_view_matrix")        static function viewMatrix(frameW:Int, frameH:Int, winW:Int, winH:Int, zoom:Float, horViewPos:Float, verViewPos:Float,
                                                                  k:RawPointer<Float>, dx:RawPointer<Float>, dy:RawPointer<Float>):Int;
    @:native("jsp_display_present")    static function displayPresent(frame:RawConstPointer<cpp.Int32>, frameW:Int, frameH:Int, out:RawPointer<cpp.Int32>, winW:Int, winH:Int,
                                                                      outPitch:SizeT, k:Float, dx:Float, dy:Float, mode:Int, filter:Int, background:cpp.UInt32,
                                                                      stream:RawPointer<cpp.Void>):Int;
    // the same window area-averaged (Fit into a small window); takes no filter — jsp_display_present refuses JSP_PRESENT_AREA
    @:native("jsp_display_present_area") static function displayPresentArea(frame:RawConstPointer<cpp.Int32>, frameW:Int, frameH:Int, out:RawPointer<cpp.Int32>, winW:Int, winH:Int,
                                                                      outPitch:SizeT, k:Float, dx:Float, dy:Float, mode:Int, background:cpp.UInt32,
                                                                      stream:RawPointer<cpp.Void>):Int;
    // the MSVideo1 16-bit encoder: frames from any pictures in device memory, two launches per slice of pictures (no codec involved)
    @:native("jsp_msv1_encoder_create")  static function msv1EncoderCreate(device:Int, w:Int, h:Int):RawPointer<JspEncoder>;
    @:native("jsp_msv1_encoder_destroy") static function msv1EncoderDestroy(e:RawPointer<JspEncoder>):Void;
    @:native("jsp_msv1_encode_bound")    static function msv1EncodeBound(e:RawPointer<JspEncoder>, bytes:RawPointer<SizeT>):Int;
    @:native("jsp_msv1_encode_frames")   static function msv1EncodeFrames(e:RawPointer<JspEncoder>, n:Int, pictures:RawConstPointer<RawConstPointer<cpp.Int32>>,
                                                                       previous:RawConstPointer<RawConstPointer<cpp.Int32>>, pitch:cpp.Int64,
                                                                       out:RawPointer<UInt8>, cap:SizeT, lens:RawPointer<SizeT>, total:RawPointer<SizeT>,
                                                                       stream:RawPointer<cpp.Void>):Int;
    @:native("jsp_frames_differ")      static function framesDiffer(a:RawConstPointer<cpp.Int32>, b:RawConstPointer<cpp.Int32>, firstPixel:SizeT, npixels:SizeT, differ:RawPointer<Int>, stream:RawPointer<cpp.Void>):Int;
}

@:include("jsplayer_amd.h") @:native("jsp_codec") @:structAccess extern class JspCodec {}
@:include("jsplayer_amd.h") @:native("jsp_index") @:structAccess extern class JspIndex {}
@:include("jsplayer_amd.h") @:native("jsp_sp_index") @:structAccess extern class JspSpIndex {}
@:include("jsplayer_amd.h") @:native("jsp_pool") @:structAccess extern class JspPool {}
@:include("jsplayer_amd.h") @:native("jsp_encoder") @:structAccess extern class JspEncoder {}
#end
