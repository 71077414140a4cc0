"""GRSS2013 (2013 IEEE GRSS Data Fusion Contest, Houston; reference loader/GRSS2013DataLoader.py): a 144-band CASI
raster plus one LiDAR height band on the same grid, 15 classes, training and validation samples in two label rasters,
a shadow map for the shadow augmenters.  The rasters are classic TIFFs in any layout common/tiff_io.py reads (strips
or tiles, chunky or planar, either byte order, uncompressed / PackBits / LZW / Deflate, Predictor 1-3; BigTIFF, JPEG
and the other codecs are refused by name).  With a compute backend the two scene rasters are decoded and the scene is
prepared on the device (tiff_io.read_raster, common/device_scene.py); the label rasters are read on the host."""
from functools import partial

import numpy

from hypelcnn_amd.common.common_nn_ops import load_shadow_map_common, read_targets_from_image, \
    shuffle_test_data_using_ratio
from hypelcnn_amd.common import device_scene
from hypelcnn_amd.common.device_scene import make_basic_data_set
from hypelcnn_amd.loader.DataLoader import DataLoader, SampleSet

CLASS_COLORS = [
    (0, 180, 0),      # healthy grass
    (0, 124, 0),      # stressed grass
    (0, 137, 69),     # synthetic grass
    (0, 69, 0),       # trees
    (172, 125, 11),   # soil
    (0, 190, 194),    # water
    (120, 0, 0),      # residential
    (216, 217, 247),  # commercial
    (121, 121, 121),  # road
    (205, 172, 127),  # highway
    (220, 175, 120),  # railway
    (100, 100, 100),  # parking lot 1
    (185, 175, 94),   # parking lot 2
    (0, 237, 0),      # tennis court
    (207, 18, 56),    # running track
]
GAN_CHECKPOINTS = {"cycle_gan": "shadow_gen_model/cycle_gan/model.ckpt-5000",
                   "dcl_gan": "shadow_gen_model/dcl_gan/model.ckpt-3000",
                   "dcl_cycle_gan": "shadow_gen_model/dcl_cycle_gan/model.ckpt-5000"}


def shadow_creators(model_base_dir, checkpoints, shadow_ratio, bands, lidar_passthrough=True, backend=None):
    """The shadow_creator_dict every shadow-capable loader registers: the three generator-based augmenters (built
    lazily, from the published checkpoints under the data directory) and the per-band ratio one."""
    from hypelcnn_amd.gan.gan_utilities import create_gan_struct, create_simple_shadow_struct
    from hypelcnn_amd.gan.shadow_data_models import shadowdata_generator_model
    from hypelcnn_amd.gan.wrappers.cycle_gan_wrapper import CycleGANInferenceWrapper
    generator_fn = partial(shadowdata_generator_model, create_only_encoder=False, is_training=False)
    creators = {name: create_gan_struct(CycleGANInferenceWrapper(generator_fn), model_base_dir, ckpt, bands=bands,
                                        backend=backend)
                for name, ckpt in checkpoints.items()}
    creators["simple"] = create_simple_shadow_struct(shadow_ratio, lidar_passthrough=lidar_passthrough)
    return creators


class GRSS2013DataLoader(DataLoader):

    def __init__(self, base_dir):
        self.base_dir = base_dir
        self.backend = None  # scene preparation: this backend, else a visible HIP device, else the host

    def get_model_base_dir(self):
        return self.base_dir + "/2013_DFTC/"

    def load_data(self, neighborhood, normalize):
        from hypelcnn_amd.common.tiff_io import read_raster
        backend = device_scene.resolve_scene_backend(self.backend)
        casi = read_raster(self.get_model_base_dir() + "2013_IEEE_GRSS_DF_Contest_CASI.tif", backend)
        lidar = read_raster(self.get_model_base_dir() + "2013_IEEE_GRSS_DF_Contest_LiDAR.tif", backend)[:, :, numpy.newaxis]
        data_set = make_basic_data_set(backend, shadow_creator_dict=None, casi=casi, lidar=lidar,
                                       neighborhood=neighborhood, normalize=normalize)
        _, shadow_ratio = self.load_shadow_map(neighborhood, data_set)
        data_set.shadow_creator_dict = shadow_creators(self.get_model_base_dir(), GAN_CHECKPOINTS, shadow_ratio,
                                                       casi.shape[2], backend=self.backend)
        return data_set

    def load_shadow_map(self, neighborhood, data_set):
        return load_shadow_map_common(data_set, neighborhood, self.get_model_base_dir() + "shadow_map.tif")

    def load_samples(self, train_data_ratio, test_data_ratio):
        """The contest's own split: TR raster -> training (a stratified share of it -> test), VA raster -> validation."""
        train_set = self.read_targets("2013_IEEE_GRSS_DF_Contest_Samples_TR.tif")
        validation_set = self.read_targets("2013_IEEE_GRSS_DF_Contest_Samples_VA.tif")
        test_set, train_set = shuffle_test_data_using_ratio(train_set, test_data_ratio)
        return SampleSet(training_targets=train_set, test_targets=test_set, validation_targets=validation_set)

    def read_targets(self, target_image_path):
        from hypelcnn_amd.common.tiff_io import imread
        return read_targets_from_image(imread(self.get_model_base_dir() + target_image_path), self.get_class_count())

    def get_class_count(self):
        return range(0, 15)

    def get_samples_color_list(self):
        return numpy.asarray(CLASS_COLORS, dtype=numpy.uint8)

    def get_band_measurements(self):
        return numpy.linspace(380, 1050, num=144)
