"""AVON (SHARE 2012, Avon NY; reference loader/AVONDataLoader.py): a 360-band hyperspectral raster without LiDAR, two
target classes marked in BMP masks (lit and shadowed occurrences of each).  The scene file stores [band, column, row]
with 55 blank entries at both ends of the row axis: the loader windows that axis and swaps the outer axes -- as a
VIEW, which the device path reads in place through strides.  Every band is clipped at its 95th percentile over the
scene before normalisation (minimum fixed at 0).  `load_shadow_corrected` switches to the shadow-corrected product,
which is stored [row, column, band] already.  The scene files may have any layout common/tiff_io.py reads; with a
compute backend they are decoded on the device (tiff_io.read_raster) and the window and the axis swap are views of the
raster there."""
import numpy

from hypelcnn_amd.common.common_nn_ops import load_shadow_map_common, read_targets_from_image, \
    shuffle_test_data_using_ratio, shuffle_training_data_using_size
from hypelcnn_amd.common import device_scene
from hypelcnn_amd.common.device_scene import make_basic_data_set
from hypelcnn_amd.loader.DataLoader import DataLoader, SampleSet
from hypelcnn_amd.loader.GRSS2013DataLoader import shadow_creators

BLANK_OFFSET = 55
SCENE = "0920-1857.georef_cropped"
GAN_CHECKPOINTS = {"cycle_gan": "shadow_gen_model/cycle_gan/model.ckpt-7000",
                   "dcl_gan": "shadow_gen_model/dcl_gan/model.ckpt-6000",
                   "dcl_cycle_gan": "shadow_gen_model/dcl_cycle_gan/model.ckpt-3000"}


class AVONDataLoader(DataLoader):

    def __init__(self, base_dir):
        self.base_dir = base_dir
        self.load_shadow_corrected = False
        self.backend = None  # scene preparation: this backend, else a visible HIP device, else the host

    def get_model_base_dir(self):
        return self.base_dir + "/AVON/"

    def load_data(self, neighborhood, normalize):
        from hypelcnn_amd.common.tiff_io import read_raster
        backend = device_scene.resolve_scene_backend(self.backend)
        if self.load_shadow_corrected:
            casi = read_raster(self.get_model_base_dir() + SCENE + "_shcorrected.tif", backend)
        else:
            casi = read_raster(self.get_model_base_dir() + SCENE + ".tif", backend)[:, :, BLANK_OFFSET:-BLANK_OFFSET]
            casi = casi.swapaxes(0, 2)
        if casi.dtype != numpy.uint16:  # (not a contest file: converted on the host, as the reference does, and uploaded)
            casi = numpy.asarray(casi).astype(numpy.uint16)
        data_set = make_basic_data_set(backend, shadow_creator_dict=None, casi=casi, lidar=None,
                                       neighborhood=neighborhood, normalize=normalize, casi_min=0, clip_percentile=95)
        _, shadow_ratio = self.load_shadow_map(neighborhood, data_set)
        # no LiDAR channel behind the bands: the ratio augmenter must not append its pass-through 1
        data_set.shadow_creator_dict = shadow_creators(self.get_model_base_dir(), GAN_CHECKPOINTS, shadow_ratio,
                                                       casi.shape[2], lidar_passthrough=False, backend=self.backend)
        return data_set

    def load_shadow_map(self, neighborhood, data_set):
        return load_shadow_map_common(data_set, neighborhood, self.get_model_base_dir() + SCENE + "_shadow.tif")

    def load_samples(self, train_data_ratio, test_data_ratio):
        """Lit occurrences of the two targets are split into training / validation; the shadowed occurrences all go to
        validation, in front; a stratified share of the training rows becomes the test set."""
        lit = [self.read_each_target(f"{SCENE}_rgb_with_targets_{no}_nsh.bmp", target_no=no) for no in (1, 2)]
        shadowed = [self.read_each_target(f"{SCENE}_rgb_with_targets_{no}_sh.bmp", target_no=no) for no in (1, 2)]
        if train_data_ratio < 1.0:
            # (the reference splits with the TEST splitter here: its first result is the share, its second the rest)
            splits = [shuffle_test_data_using_ratio(rows, train_data_ratio) for rows in lit]
        else:
            splits = [shuffle_training_data_using_size(self.get_class_count(), rows, int(train_data_ratio), None)
                      for rows in lit]
        train_set = numpy.vstack([s[0] for s in splits])
        validation_set = numpy.vstack(shadowed + [s[1] for s in splits])
        test_set, train_set = shuffle_test_data_using_ratio(train_set, test_data_ratio)
        return SampleSet(training_targets=train_set, test_targets=test_set, validation_targets=validation_set)

    def read_each_target(self, target_image_path, target_no):
        """A mask marks one target in white (a 1-bit file: True): its pixels get label target_no - 1, every other
        pixel -1, which is no class.  The blank rows at both ends of the mask are dropped first."""
        from hypelcnn_amd.common.bmp_io import imread
        mask = imread(self.get_model_base_dir() + target_image_path)
        mask = mask[BLANK_OFFSET:mask.shape[0] - BLANK_OFFSET]
        marked = mask if mask.dtype == bool else mask == 255
        return read_targets_from_image(numpy.where(marked, target_no - 1, -1), self.get_class_count())

    def read_targets(self, target_image_path):
        from hypelcnn_amd.common.tiff_io import imread
        return read_targets_from_image(imread(self.get_model_base_dir() + target_image_path), self.get_class_count())

    def get_class_count(self):
        return range(0, 2)

    def get_samples_color_list(self):
        return numpy.asarray([(0, 0, 255), (255, 0, 0)], dtype=numpy.uint8)

    def get_band_measurements(self):
        return numpy.linspace(400, 2500, num=360)
