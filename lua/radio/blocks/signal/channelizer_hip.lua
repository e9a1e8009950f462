---
-- PolyphaseChannelizerBlock: a critically sampled K-channel analysis filterbank (BASELINE.json configs[4]).  NOT a block of the reference - there is no
-- channelizer under radio/blocks/ - so this file is a whole block, not a patch: tools/apply_lua_binding.py copies it to
-- radio/blocks/signal/channelizer_hip.lua and a script reaches it as
--
--     local PolyphaseChannelizerBlock = require('radio.blocks.signal.channelizer_hip').PolyphaseChannelizerBlock
--     top:connect(source, PolyphaseChannelizerBlock(64, taps), sink)
--
-- It is defined by reference blocks: K parallel chains FrequencyTranslatorBlock(-c * rate / K) -> FIRFilterBlock(taps) -> DownsamplerBlock(K),
-- c = 0 .. K-1, evaluated as ONE dense GEMM on the f32 matrix cores (lrhip_channelizer_create).  Output: frames of K ComplexFloat32 values, channel c at
-- position c of its frame, one frame per K input samples - so the port carries rate samples per second in total and each channel runs at rate / K.
-- K in {32, 64}; #taps a multiple of 32.  Without the library the constructor raises (there is no host implementation to fall back to).
--
-- options.method = "fft" evaluates the same filterbank in its polyphase + FFT form (lrhip_pfb_channelizer_create): K a power of two in [8, 4096],
-- K <= #taps <= min(64 K, 65536), ~50x less arithmetic.  "gemm" asks for the GEMM.  Without a method the GEMM runs where it accepts the shape
-- and the FFT form everywhere else.
--
-- options.oversample = 2 or 4 makes the hop D = K / oversample instead of K: one frame per D input samples, each channel at oversample * rate / K and
-- the port at oversample * rate, so that the prototype's skirt past rate / (2 K) no longer aliases into the channel and a carrier between two
-- channel centres comes out clean of either neighbour.  Frame m * oversample is frame m of the critically sampled bank.  The FFT form only
-- (lrhip_pfb_oversampled_create); "gemm" with oversample > 1 raises.
--
-- @block PolyphaseChannelizerBlock
-- @tparam int num_channels Number of channels K
-- @tparam array|vector taps Real-valued prototype lowpass taps (e.g. radio.utilities.filter_utils.firwin_lowpass(16 * K, 1 / K))
-- @tparam[opt={}] table options Additional options, specifying:
--                         * `method` (string, "gemm" or "fft")
--                         * `oversample` (int, 1, 2 or 4; default 1)

local ffi = require('ffi')

local block = require('radio.core.block')
local types = require('radio.types')
local lrhip = require('radio.core.lrhip')

local PolyphaseChannelizerBlock = block.factory("PolyphaseChannelizerBlock")

function PolyphaseChannelizerBlock:instantiate(num_channels, taps, options)
    assert(lrhip.available, "PolyphaseChannelizerBlock needs liblrhip.so")
    self.num_channels = assert(num_channels, "Missing argument #1 (num_channels)")
    assert(taps, "Missing argument #2 (taps)")
    if type(taps) == "table" and taps.data_type == nil then
        self.taps = types.Float32.vector_from_array(taps)
    else
        assert(taps.data_type == types.Float32, "Unsupported taps type")
        self.taps = taps
    end
    self.method = (options or {}).method
    assert(self.method == nil or self.method == "gemm" or self.method == "fft", "Unsupported method (\"gemm\" or \"fft\")")
    self.oversample = (options or {}).oversample or 1
    assert(self.oversample == 1 or self.oversample == 2 or self.oversample == 4, "Unsupported oversample (1, 2 or 4)")
    assert(self.oversample == 1 or self.method ~= "gemm", "oversample > 1 needs the FFT form: the GEMM (method = \"gemm\") is critically sampled only")
    self:add_type_signature({block.Input("in", types.ComplexFloat32)}, {block.Output("out", types.ComplexFloat32)})
end

function PolyphaseChannelizerBlock:get_rate()
    return block.Block.get_rate(self) * self.oversample
end

function PolyphaseChannelizerBlock:initialize()
    self.out = types.ComplexFloat32.vector()
end

---
-- PolyphaseSynthesizerBlock: the synthesis filterbank that undoes the channelizer - K parallel chains UpsamplerBlock(D) -> FIRFilterBlock(taps) ->
-- FrequencyTranslatorBlock(+c * rate_out / K), c = 0 .. K-1, summed, D = K / oversample - in its polyphase + FFT form.  Input: the frame stream the
-- channelizer emits (K ComplexFloat32 values per frame, channel c at position c; a vector may end inside a frame, whose values wait for the next one);
-- output: D samples per completed frame, so the port carries rate / oversample samples per second.  K a power of two in [8, 4096],
-- K <= #taps <= min(64 K, 65536).  The stage has no entry point of its own: it is created by name through lrhip_unary_create, its taps travelling in
-- the name as %.9g text, which gives every Float32 back exactly.
--
--     local PolyphaseSynthesizerBlock = require('radio.blocks.signal.channelizer_hip').PolyphaseSynthesizerBlock
--     top:connect(channelizer, PolyphaseSynthesizerBlock(64, taps, {oversample = 2}), sink)
--
-- @block PolyphaseSynthesizerBlock
-- @tparam int num_channels Number of channels K
-- @tparam array|vector taps Real-valued prototype lowpass taps
-- @tparam[opt={}] table options Additional options, specifying:
--                         * `oversample` (int, 1, 2 or 4; default 1)

local PolyphaseSynthesizerBlock = block.factory("PolyphaseSynthesizerBlock")

function PolyphaseSynthesizerBlock:instantiate(num_channels, taps, options)
    assert(lrhip.available, "PolyphaseSynthesizerBlock needs liblrhip.so")
    self.num_channels = assert(num_channels, "Missing argument #1 (num_channels)")
    assert(taps, "Missing argument #2 (taps)")
    if type(taps) == "table" and taps.data_type == nil then
        self.taps = types.Float32.vector_from_array(taps)
    else
        assert(taps.data_type == types.Float32, "Unsupported taps type")
        self.taps = taps
    end
    self.oversample = (options or {}).oversample or 1
    assert(self.oversample == 1 or self.oversample == 2 or self.oversample == 4, "Unsupported oversample (1, 2 or 4)")
    self:add_type_signature({block.Input("in", types.ComplexFloat32)}, {block.Output("out", types.ComplexFloat32)})
end

function PolyphaseSynthesizerBlock:get_rate()
    return block.Block.get_rate(self) / self.oversample
end

function PolyphaseSynthesizerBlock:initialize()
    self.out = types.ComplexFloat32.vector()
end

-- "pfbsynthesizer:channels=K:oversample=R:taps=v,v,..." (include/lrhip.h)
function PolyphaseSynthesizerBlock:op()
    local text = {}
    for i = 0, self.taps.length - 1 do
        text[i + 1] = string.format("%.9g", self.taps.data[i].value)
    end
    return string.format("pfbsynthesizer:channels=%d:oversample=%d:taps=", self.num_channels, self.oversample) .. table.concat(text, ",")
end

local M = {PolyphaseChannelizerBlock = PolyphaseChannelizerBlock, PolyphaseSynthesizerBlock = PolyphaseSynthesizerBlock}

-- Does this liblrhip.so have the FFT form?  These files are copied into a LuaRadio checkout and may meet an older library there; LuaJIT raises on the
-- first index of a symbol the library lacks.  So the entry point is called once, when this file loads, with a shape it refuses before it looks at the
-- device (no channels: a null result, nothing created, no device context).  Without it the block is the GEMM alone, as it was.
M.has_fft = lrhip.available and pcall(function ()
    return lrhip.lib.lrhip_pfb_channelizer_create(nil, 0, 0)
end)

-- The oversampled form, asked for in the same way (an oversample of 0 is refused before anything else is looked at).
M.has_oversampled = lrhip.available and pcall(function ()
    return lrhip.lib.lrhip_pfb_oversampled_create(nil, 0, 0, 0)
end)

-- create: the block's stage constructor; without one, the channelizer's choice among its three entry points
function M.patch(Block, create)
    lrhip.device_block(Block, create or function (self)
        local k, m = self.num_channels, self.taps.length
        if self.oversample > 1 then
            assert(M.has_oversampled, "this liblrhip.so has no lrhip_pfb_oversampled_create (oversample = " .. self.oversample .. ")")
            return lrhip.lib.lrhip_pfb_oversampled_create(ffi.cast("const float *", self.taps.data), m, k, self.oversample)
        end
        local gemm_accepts = (k == 32 or k == 64) and m >= 32 and m <= 8192 and m % 32 == 0
        assert(self.method ~= "fft" or M.has_fft, "this liblrhip.so has no lrhip_pfb_channelizer_create (method = \"fft\")")
        if M.has_fft and (self.method == "fft" or (self.method == nil and not gemm_accepts)) then
            return lrhip.lib.lrhip_pfb_channelizer_create(ffi.cast("const float *", self.taps.data), self.taps.length, self.num_channels)
        end
        return lrhip.lib.lrhip_channelizer_create(ffi.cast("const float *", self.taps.data), self.taps.length, self.num_channels)
    end)
    function Block:process(x)
        return lrhip.execute(self:create_stage(), x, self.out, self)
    end
end

M.patch(PolyphaseChannelizerBlock)
M.patch(PolyphaseSynthesizerBlock, function (self)
    return lrhip.lib.lrhip_unary_create(self:op(), 0, 0, 0, 1)
end)

return M
